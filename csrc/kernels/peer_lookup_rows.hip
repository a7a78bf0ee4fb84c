// Peer lookup on row-wise sharded tables (ModelConfig.embedding_sharding: row
// with embedding_exchange: peer, and mixed plans). A table is cut into one
// contiguous row range per rank (launchers.h PeerLookupArgs rlo / roff); each
// lane finds the rank that holds its row (peer_lookup.h range_row_bytes: world
// - 1 compares, no division) and loads it there - this rank's store, a peer's
// IPC-mapped store, or the replica cache. Nothing is masked or reduced, and a
// bag's ids may live on different ranks. Keys ((t << 40) | global row), the
// cache index, the counters and the ring sampling are peer_lookup.h unchanged;
// "remote" is per lookup, no longer per table.
//
// Each kernel is its table-wise twin with only the row locator exchanged: the
// same lane layout, the same order of loads and atomics, the same LDS use.
//   dot_interact_gather_peer_rows_kernel      mirrors dot_interact_gather_kernel, peer branch (interaction.hip)
//   dot_interact_gather_peer_rows_fp8_kernel  mirrors dot_interact_gather_peer_fp8_kernel (peer_lookup_fp8.hip)
//   peer_bag_rows_kernel                      mirrors peer_bag_kernel (peer_lookup.hip)
//   peer_bag_rows_fp8_kernel                  mirrors peer_bag_fp8_kernel (peer_lookup_fp8.hip)
//   peer_cache_fill_rows_kernel<128>          mirrors peer_cache_fill_kernel (peer_lookup.hip)
//   peer_cache_fill_rows_kernel<64>           mirrors peer_cache_fill_fp8_kernel (peer_lookup_fp8.hip)
// The twins stay apart so that their compiled resources do not move.
#include "common.h"
#include "fp8_rows.h"
#include "launchers.h"
#include "peer_lookup.h"

namespace dtfs {
namespace kern {

// K1 + K5, bf16 rows: one wave per candidate, lane (r, h), r = 1..T reads its
// table's row where the ranges put it.
template <typename IdT>
__global__ void __launch_bounds__(256) dot_interact_gather_peer_rows_kernel(
    const bf16* __restrict__ dense, int64_t ldd, const IdT* __restrict__ ids, int64_t ldi, int T, int B,
    bf16* __restrict__ out, int64_t ldo, int out_cols, const uint8_t* __restrict__ arena, int id_col0,
    PeerLookupArgs peer) {
  constexpr int D = 64;
  constexpr int ROWB = 4 * 2048;  // LDS bytes per block: 4 waves x one output row (<= 1024 columns)
  __shared__ __attribute__((aligned(16))) uint8_t lds[ROWB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * (blockDim.x / 64) + w;
  if (b >= B) return;
  const int r = lane & 31, h = lane >> 5;
  const int nv = T + 1;
  const bf16* src = nullptr;
  int hit = -1;
  int64_t key = 0;
  if (r >= 1 && r < nv) {
    const int t = r - 1;
    const int64_t m = range_table_rows(peer, t);
    int64_t id = 0;
    if (arena) {  // the request arena's row b (K0 fused: no unpack pass); padding rows read id 0
      const ArenaRow ar = arena_row(arena, kArenaPayloadOff, b);
      float w;
      if (ar.ids) arena_feature(ar, id_col0 + t, id, w);
    } else {
      id = int64_t(ids[int64_t(b) * ldi + t]);
    }
    int64_t v = id % m;
    if (v < 0) v += m;
    src = reinterpret_cast<const bf16*>(range_peer_row_bytes<kRowBytesBf16>(peer, cache_view(peer), t, v, hit));
    key = (int64_t(t) << 40) | v;
  }
  // wave-uniform branches; converged: the ballots see every lane
  if (peer_counted(peer, b)) peer_count(peer, hit, h == 0);  // lanes h = 1 repeat h = 0's rows
  if (peer.sample_every > 0 && peer_sampled(peer, b)) ring_push(peer, key, h == 0 && hit >= 0);
  bf16x8 x[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int k = 16 * s + 8 * h;
    x[s] = bf16x8{};
    if (r == 0) x[s] = *reinterpret_cast<const bf16x8*>(dense + int64_t(b) * ldd + k);
    else if (src) x[s] = *reinterpret_cast<const bf16x8*>(src + k);
  }
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[s], x[s], acc, 0, 0, 0);
  // assemble the row in this wave's LDS slice: [dense | lower triangle | zeros]
  bf16* o = reinterpret_cast<bf16*>(lds + w * (ROWB / 4));
  const int n8 = out_cols / 8;
  for (int c = lane; c < n8; c += 64) *reinterpret_cast<bf16x8*>(o + c * 8) = bf16x8{};
  __builtin_amdgcn_wave_barrier();
  if (lane < D / 8) *reinterpret_cast<bf16x8*>(o + lane * 8) = *reinterpret_cast<const bf16x8*>(dense + int64_t(b) * ldd + lane * 8);
  const int col = lane & 31;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int rowi = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
    if (rowi < nv && col < rowi) o[D + rowi * (rowi - 1) / 2 + col] = f2bf(acc[reg]);
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  bf16* dst = out + int64_t(b) * ldo;
  for (int c = lane; c < n8; c += 64) *reinterpret_cast<bf16x8*>(dst + c * 8) = *reinterpret_cast<const bf16x8*>(o + c * 8);
}

// K1 + K5, e4m3 code rows: every load unconditional, the four 8-byte code
// loads issued before the counters' atomics and the first MFMA, the dense
// vector through the wave's LDS row. Lanes without a table row load from the
// candidate's own dense row (always mapped, 128 valid bytes) and are masked
// after the load.
template <typename IdT>
__global__ void __launch_bounds__(256) dot_interact_gather_peer_rows_fp8_kernel(
    const bf16* __restrict__ dense, int64_t ldd, const float* __restrict__ tscale, const IdT* __restrict__ ids,
    int64_t ldi, int T, int B, bf16* __restrict__ out, int64_t ldo, int out_cols, const uint8_t* __restrict__ arena,
    int id_col0, PeerLookupArgs peer) {
  constexpr int D = 64;
  constexpr int ROWB = 4 * 2048;  // LDS bytes per block: 4 waves x one output row (<= 1024 columns)
  __shared__ __attribute__((aligned(16))) uint8_t lds[ROWB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * (blockDim.x / 64) + w;
  if (b >= B) return;
  const int r = lane & 31, h = lane >> 5;
  const int nv = T + 1;
  const bf16* drow = dense + int64_t(b) * ldd;
  // the dense row's chunk lane & 7 (lanes 8.. repeat the same 128 bytes: no branch around the load)
  const bf16x8 dv = *reinterpret_cast<const bf16x8*>(drow + (lane & 7) * 8);
  const bool has_row = r >= 1 && r < nv;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(drow);
  float sc = 1.f;
  int hit = -1;
  int64_t key = 0;
  if (has_row) {
    const int t = r - 1;
    const int64_t m = range_table_rows(peer, t);
    int64_t id = 0;
    if (arena) {  // the request arena's row b (K0 fused: no unpack pass); padding rows read id 0
      const ArenaRow ar = arena_row(arena, kArenaPayloadOff, b);
      float w;
      if (ar.ids) arena_feature(ar, id_col0 + t, id, w);
    } else {
      id = int64_t(ids[int64_t(b) * ldi + t]);
    }
    int64_t v = id % m;
    if (v < 0) v += m;
    src = range_peer_row_bytes<kRowBytesFp8>(peer, cache_view(peer), t, v, hit);
    key = (int64_t(t) << 40) | v;
    sc = tscale[t];
  }
  uint2 q[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) q[s] = *reinterpret_cast<const uint2*>(src + 16 * s + 8 * h);
  // wave-uniform branches; converged: the ballots see every lane
  if (peer_counted(peer, b)) peer_count(peer, hit, h == 0);  // lanes h = 1 repeat h = 0's rows
  if (peer.sample_every > 0 && peer_sampled(peer, b)) ring_push(peer, key, h == 0 && hit >= 0);
  // the row's first 64 columns = the dense vector, in this wave's LDS slice
  bf16* o = reinterpret_cast<bf16*>(lds + w * (ROWB / 4));
  if (lane < D / 8) *reinterpret_cast<bf16x8*>(o + lane * 8) = dv;
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  bf16x8 xd[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) xd[s] = *reinterpret_cast<const bf16x8*>(o + 16 * s + 8 * h);
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    // lanes past the last table hold code 0 = +0.0
    const uint2 qs = has_row ? q[s] : make_uint2(0u, 0u);
    const bf16x8 xc = fp8x8_to_bf16(qs, sc);
    const bf16x8 x = r == 0 ? xd[s] : xc;
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, x, acc, 0, 0, 0);
  }
  // assemble the rest of the row behind the dense columns: [lower triangle | zeros]
  const int n8 = out_cols / 8;
  for (int c = D / 8 + lane; c < n8; c += 64) *reinterpret_cast<bf16x8*>(o + c * 8) = bf16x8{};
  __builtin_amdgcn_wave_barrier();
  const int col = lane & 31;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int rowi = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
    if (rowi < nv && col < rowi) o[D + rowi * (rowi - 1) / 2 + col] = f2bf(acc[reg]);
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  bf16* dst = out + int64_t(b) * ldo;
  for (int c = lane; c < n8; c += 64) *reinterpret_cast<bf16x8*>(dst + c * 8) = *reinterpret_cast<const bf16x8*>(o + c * 8);
}

// K1b, bf16 rows. 8 lanes per (candidate b, table t): lane c of the group owns
// columns 8c .. 8c + 7 of the pooled row, accumulated in fp32 over the bag's
// ids - each id's row from whichever rank's range holds it.
template <typename IdT>
__global__ void __launch_bounds__(256) peer_bag_rows_kernel(PeerLookupArgs p, const IdT* __restrict__ ids, int64_t ldi,
                                                            const float* __restrict__ wts, int64_t ldw,
                                                            const uint8_t* __restrict__ arena, int col0, int T,
                                                            int hot, int B, bf16* __restrict__ out) {
  const int64_t q = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 3;
  const int c = threadIdx.x & 7;
  const bool valid = q < int64_t(B) * T;
  const int b = valid ? int(q / T) : 0, t = valid ? int(q % T) : 0;
  const CacheView cv = cache_view(p);
  ArenaRow ar{nullptr, nullptr, false, kArenaAllWeights, 4};
  if (arena && valid) ar = arena_row(arena, kArenaPayloadOff, b);
  const int64_t m = range_table_rows(p, t);
  const bool sample = valid && c == 0 && p.sample_every > 0 && peer_sampled(p, b);
  const bool counted = valid && c == 0 && peer_counted(p, b);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < hot; ++j) {  // uniform trip count: the ballots below see every lane
    const int col = col0 + t * hot + j;
    int64_t id = 0;
    float w = 0.f;
    if (valid) {
      if (arena) {
        if (ar.ids) arena_feature(ar, col, id, w);
      } else {
        id = int64_t(ids[int64_t(b) * ldi + col]);
        w = wts[int64_t(b) * ldw + col];
      }
    }
    int64_t v = id % m;
    if (v < 0) v += m;
    int hit = -1;
    const bf16* src = reinterpret_cast<const bf16*>(range_peer_row_bytes<kRowBytesBf16>(p, cv, t, v, hit));
    if (valid) {
      const bf16x8 x = *reinterpret_cast<const bf16x8*>(src + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += w * bf2f(x[e]);
    }
    peer_count(p, hit, counted);
    ring_push(p, (int64_t(t) << 40) | v, sample && hit >= 0);
  }
  if (valid) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(acc[e]);
    *reinterpret_cast<bf16x8*>(out + q * 64 + c * 8) = o;
  }
}

// K1b, e4m3 code rows: lane c of the group reads the 8 code bytes of columns
// 8c .. 8c + 7 and accumulates (float(code) * tscale[t]) * w in fp32.
template <typename IdT>
__global__ void __launch_bounds__(256) peer_bag_rows_fp8_kernel(PeerLookupArgs p, const float* __restrict__ tscale,
                                                                const IdT* __restrict__ ids, int64_t ldi,
                                                                const float* __restrict__ wts, int64_t ldw,
                                                                const uint8_t* __restrict__ arena, int col0, int T,
                                                                int hot, int B, bf16* __restrict__ out) {
  const int64_t q = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 3;
  const int c = threadIdx.x & 7;
  const bool valid = q < int64_t(B) * T;
  const int b = valid ? int(q / T) : 0, t = valid ? int(q % T) : 0;
  const CacheView cv = cache_view(p);
  ArenaRow ar{nullptr, nullptr, false, kArenaAllWeights, 4};
  if (arena && valid) ar = arena_row(arena, kArenaPayloadOff, b);
  const int64_t m = range_table_rows(p, t);
  const float sc = tscale[t];
  const bool sample = valid && c == 0 && p.sample_every > 0 && peer_sampled(p, b);
  const bool counted = valid && c == 0 && peer_counted(p, b);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < hot; ++j) {  // uniform trip count: the ballots below see every lane
    const int col = col0 + t * hot + j;
    int64_t id = 0;
    float w = 0.f;
    if (valid) {
      if (arena) {
        if (ar.ids) arena_feature(ar, col, id, w);
      } else {
        id = int64_t(ids[int64_t(b) * ldi + col]);
        w = wts[int64_t(b) * ldw + col];
      }
    }
    int64_t v = id % m;
    if (v < 0) v += m;
    int hit = -1;
    const uint8_t* src = range_peer_row_bytes<kRowBytesFp8>(p, cv, t, v, hit);
    if (valid) {
      const uint2 x = *reinterpret_cast<const uint2*>(src + c * 8);
      const f32x2 f[4] = {__builtin_amdgcn_cvt_pk_f32_fp8(int(x.x), false), __builtin_amdgcn_cvt_pk_f32_fp8(int(x.x), true),
                          __builtin_amdgcn_cvt_pk_f32_fp8(int(x.y), false), __builtin_amdgcn_cvt_pk_f32_fp8(int(x.y), true)};
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += (f[e >> 1][e & 1] * sc) * w;
    }
    peer_count(p, hit, counted);
    ring_push(p, (int64_t(t) << 40) | v, sample && hit >= 0);
  }
  if (valid) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(acc[e]);
    *reinterpret_cast<bf16x8*>(out + q * 64 + c * 8) = o;
  }
}

// Replica cache fill, 8 lanes per key: rows[slot] = the ROWB bytes of the
// key's table row, read where its range lives. ROWB 128: bf16 rows (16 bytes
// per lane); 64: e4m3 code rows (8 bytes per lane).
template <int ROWB>
__global__ void __launch_bounds__(256) peer_cache_fill_rows_kernel(PeerLookupArgs p, int T,
                                                                   const int64_t* __restrict__ keys,
                                                                   const int32_t* __restrict__ slots, int64_t n,
                                                                   uint8_t* __restrict__ rows, int64_t cap) {
  const int64_t i = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 3;
  const int c = threadIdx.x & 7;
  if (i >= n) return;
  const int64_t key = keys[i];
  const int64_t t = key >> 40;
  const int64_t s = slots[i];
  if (key < 0 || t >= T || s < 0 || s >= cap) return;
  const int64_t v = min(key & ((int64_t(1) << 40) - 1), range_table_rows(p, int(t)) - 1);
  int owner;
  const uint8_t* src = range_row_bytes<ROWB>(p, int(t), v, owner);
  if (ROWB == kRowBytesBf16)
    *reinterpret_cast<bf16x8*>(rows + s * ROWB + c * 16) = *reinterpret_cast<const bf16x8*>(src + c * 16);
  else
    *reinterpret_cast<uint2*>(rows + s * ROWB + c * 8) = *reinterpret_cast<const uint2*>(src + c * 8);
}

}  // namespace kern

using namespace kern;

// the range descriptor's own fields (the bindings check the ranges' contents
// against the stores on the host before any launch)
static bool peer_ranges_ok(const PeerLookupArgs& p) {
  return p.cbase && p.rlo && p.roff && p.world >= 1 && p.world <= 64 && p.rank >= 0 && p.rank < p.world &&
         p.max_chunks >= 1 && p.chunk_shift >= 1 && p.chunk_shift <= 40 && (!p.ring || (p.ring_ctr && p.ring_cap >= 64));
}

static bool fp8_chunk_ok(const float* tscale, const void* chunk0) {
  return !tscale || (chunk0 && reinterpret_cast<uintptr_t>(chunk0) % 8 == 0);
}

hipError_t launch_dot_interaction_gather_peer_rows(const void* dense, int64_t ldd, const PeerLookupArgs& p,
                                                   const float* tscale, const void* chunk0, const void* ids,
                                                   bool ids64, int64_t ldi, int T, int B, void* out, int64_t ldo,
                                                   int out_cols, hipStream_t st, const void* arena, int id_col0) {
  if (B == 0) return hipSuccess;
  if (B < 0 || T < 1 || T + 1 > 32 || out_cols % 8 || out_cols > 1024 || out_cols < 64 + (T + 1) * T / 2 || ldo % 8 ||
      ldo < out_cols || ldd % 8 || ldd < 64 || (!arena && (!ids || ldi < T)) || (arena && id_col0 < 0) ||
      !peer_ranges_ok(p) || !fp8_chunk_ok(tscale, chunk0) || !dense || !out ||
      reinterpret_cast<uintptr_t>(dense) % 16 || reinterpret_cast<uintptr_t>(out) % 16)
    return hipErrorInvalidValue;
  const uint8_t* ar = static_cast<const uint8_t*>(arena);
  const bf16* d = static_cast<const bf16*>(dense);
  bf16* o = static_cast<bf16*>(out);
  dim3 grid((B + 3) / 4), block(256);
  if (tscale) {
    if (ids64)
      hipLaunchKernelGGL(dot_interact_gather_peer_rows_fp8_kernel<int64_t>, grid, block, 0, st, d, ldd, tscale,
                         static_cast<const int64_t*>(ids), ldi, T, B, o, ldo, out_cols, ar, id_col0, p);
    else
      hipLaunchKernelGGL(dot_interact_gather_peer_rows_fp8_kernel<int32_t>, grid, block, 0, st, d, ldd, tscale,
                         static_cast<const int32_t*>(ids), ldi, T, B, o, ldo, out_cols, ar, id_col0, p);
  } else {
    if (ids64)
      hipLaunchKernelGGL(dot_interact_gather_peer_rows_kernel<int64_t>, grid, block, 0, st, d, ldd,
                         static_cast<const int64_t*>(ids), ldi, T, B, o, ldo, out_cols, ar, id_col0, p);
    else
      hipLaunchKernelGGL(dot_interact_gather_peer_rows_kernel<int32_t>, grid, block, 0, st, d, ldd,
                         static_cast<const int32_t*>(ids), ldi, T, B, o, ldo, out_cols, ar, id_col0, p);
  }
  return hipGetLastError();
}

hipError_t launch_peer_bag_rows(const PeerLookupArgs& p, const float* tscale, const void* chunk0, const void* ids,
                                bool ids64, int64_t ldi, const float* wts, int64_t ldw, const void* arena, int col0,
                                int T, int hot, int B, void* out, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (B < 0 || !peer_ranges_ok(p) || !fp8_chunk_ok(tscale, chunk0) || T < 1 || hot < 1 || col0 < 0 || !out ||
      reinterpret_cast<uintptr_t>(out) % 16 ||
      (!arena && (!ids || !wts || ldi < col0 + T * hot || ldw < col0 + T * hot)))
    return hipErrorInvalidValue;
  const int64_t threads = int64_t(B) * T * 8;
  const dim3 grid(unsigned((threads + 255) / 256)), block(256);
  const uint8_t* ar = static_cast<const uint8_t*>(arena);
  bf16* o = static_cast<bf16*>(out);
  const bool i64 = arena || ids64;
  if (tscale) {
    if (i64)
      hipLaunchKernelGGL(peer_bag_rows_fp8_kernel<int64_t>, grid, block, 0, st, p, tscale,
                         static_cast<const int64_t*>(ids), ldi, wts, ldw, ar, col0, T, hot, B, o);
    else
      hipLaunchKernelGGL(peer_bag_rows_fp8_kernel<int32_t>, grid, block, 0, st, p, tscale,
                         static_cast<const int32_t*>(ids), ldi, wts, ldw, ar, col0, T, hot, B, o);
  } else {
    if (i64)
      hipLaunchKernelGGL(peer_bag_rows_kernel<int64_t>, grid, block, 0, st, p, static_cast<const int64_t*>(ids), ldi,
                         wts, ldw, ar, col0, T, hot, B, o);
    else
      hipLaunchKernelGGL(peer_bag_rows_kernel<int32_t>, grid, block, 0, st, p, static_cast<const int32_t*>(ids), ldi,
                         wts, ldw, ar, col0, T, hot, B, o);
  }
  return hipGetLastError();
}

hipError_t launch_peer_cache_fill_rows(const PeerLookupArgs& p, int T, bool fp8, const void* chunk0,
                                       const int64_t* keys, const int32_t* slots, int64_t n, void* rows, int64_t cap,
                                       hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!peer_ranges_ok(p) || !keys || !slots || T < 1 || !rows || cap < 1 || n < 0 ||
      reinterpret_cast<uintptr_t>(rows) % (fp8 ? 8 : 16) ||
      (fp8 && (!chunk0 || reinterpret_cast<uintptr_t>(chunk0) % 8)))
    return hipErrorInvalidValue;
  const dim3 grid(unsigned((n * 8 + 255) / 256)), block(256);
  if (fp8)
    hipLaunchKernelGGL(peer_cache_fill_rows_kernel<kRowBytesFp8>, grid, block, 0, st, p, T, keys, slots, n,
                       static_cast<uint8_t*>(rows), cap);
  else
    hipLaunchKernelGGL(peer_cache_fill_rows_kernel<kRowBytesBf16>, grid, block, 0, st, p, T, keys, slots, n,
                       static_cast<uint8_t*>(rows), cap);
  return hipGetLastError();
}

}  // namespace dtfs
