// Multi-hot DLRM (ModelConfig.multi_hot > 1) on local tables: the bag pooling
// (K1b) fused into the dot interaction (K5), on bf16 tables and on the fp8 store
// (e4m3 codes + one power-of-two scale per table, interaction_fp8.hip).
//
// For candidate b, with hot ids per table and one fp32 weight per id:
//   p[t]  = bf16(sum_{j < hot} w(b, t hot + j) * row_t(id(b, t hot + j) mod m_t))   fp32, j ascending
//   X     = [dense_b ; p[0] ; ... ; p[T-1]]
//   out_b = [dense_b | strictly lower triangle of X X^T, row-major | zero pad]
// which is what pack_ids + the bag kernel (bf16 out) + dot_interact_kernel
// compute in three launches through a [B, T, 64] buffer in HBM; only the order
// of the fp32 sum inside a bag differs from the bag kernel's.
//
// Work split (the one-hot kernels'): one wave per candidate, 4 waves per block.
// Lane (r, h), r = lane & 31, h = lane >> 5: r = 0 is the dense vector, r = 1..T
// owns table r - 1; for k-step s the lane owns K positions 16 s + 8 h .. + 8, so
// its pooled values are directly its four MFMA operands.
//
// Three phases per wave, each wave on its own LDS slice (8 KB):
//   1. stage: the candidate's T hot (id, weight) pairs are read with coalesced
//      loads (lane e, e + 64, ..), or from the request arena's row; the lane
//      that reads an id also hashes it (the 64-bit modulo runs T hot / 64 times
//      per lane here, it would run hot times per lane after the transpose) and
//      leaves the clamped global table row (int64) and the weight in LDS.
//   2. pool: each lane walks its table's hot entries in batches of U: U LDS
//      reads of (row, weight), then all 4 U row-chunk loads before the first
//      FMA. U = 2 on bf16 rows (16-byte loads), U = 4 on code rows (8-byte
//      loads): 8 KB of independent random reads in flight per wave either
//      way, and both kernels stay at 4 waves per SIMD (the bf16 kernel at
//      U = 3 / 4 takes 136 / 162 VGPRs: 3 / 2 waves). Every load is
//      unconditional (see interaction_fp8.hip): lanes without a table and
//      entries past hot in the last batch read staged entry 0 with weight 0.
//      32 fp32 accumulators per lane, acc = fma(value, w, acc) in id order; the
//      fp8 kernel's value is cvt_pk_f32_fp8(code) * scale (exact), then the
//      same fma: bit-equal to the bf16 kernel on the dequantised store.
//   3. interact: pooled values -> bf16, the four v_mfma_f32_32x32x16_bf16 and
//      the LDS-assembled output row of the one-hot kernels.
//
// Limits (launcher): 1 <= T <= 31, hot >= 2, T hot <= kBagStage = 512 staged
// pairs per candidate (12 bytes each: 6 KB of the wave's slice beside the 2 KB
// output row; hot <= 16 at T = 31), out_cols as the one-hot kernels. 32 KB of
// LDS per block: 5 blocks (20 waves) per CU before registers limit it.
#include "common.h"
#include "fp8_rows.h"
#include "launchers.h"

namespace dtfs {
namespace kern {

constexpr int kBagStage = 512;  // staged (row, weight) pairs per candidate

// 8 values of a row chunk as fp32: bf16 bits << 16, or e4m3 codes * scale
template <bool FP8>
struct BagChunk;
template <>
struct BagChunk<false> {
  typedef uint4 Q;
  static constexpr int kRowBytes = 128, kStep = 32, kHalf = 16, kU = 2;
  static __device__ __forceinline__ void unpack(const Q& q, float, float (&v)[8]) {
    const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(d[i] << 16);
      v[2 * i + 1] = __uint_as_float(d[i] & 0xffff0000u);
    }
  }
};
template <>
struct BagChunk<true> {
  typedef uint2 Q;
  static constexpr int kRowBytes = 64, kStep = 16, kHalf = 8, kU = 4;
  static __device__ __forceinline__ void unpack(const Q& q, float sc, float (&v)[8]) {
    const f32x2 p[4] = {__builtin_amdgcn_cvt_pk_f32_fp8(int(q.x), false), __builtin_amdgcn_cvt_pk_f32_fp8(int(q.x), true),
                        __builtin_amdgcn_cvt_pk_f32_fp8(int(q.y), false), __builtin_amdgcn_cvt_pk_f32_fp8(int(q.y), true)};
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = p[i >> 1][i & 1] * sc;
  }
};

// id -> python-style non-negative id mod m; ids and moduli below 2^32 (every
// host-narrowed request) skip the 64-bit software division
__device__ __forceinline__ int64_t bag_mod(int64_t id, int64_t m) {
  if (((uint64_t(id) | uint64_t(m)) >> 32) == 0) return int64_t(uint32_t(id) % uint32_t(m));
  const int64_t v = id % m;
  return v < 0 ? v + m : v;
}

template <bool FP8, typename IdT>
__device__ __forceinline__ void dot_interact_bag_body(
    const bf16* __restrict__ dense, int64_t ldd, const uint8_t* __restrict__ table, int64_t table_rows,
    const float* __restrict__ scale, const IdT* __restrict__ ids, int64_t ldi, const float* __restrict__ wts,
    int64_t ldw, int hot, const int64_t* __restrict__ modulo_f, const int64_t* __restrict__ offset_f, int T, int B,
    bf16* __restrict__ out, int64_t ldo, int out_cols, const uint8_t* __restrict__ arena, int id_col0) {
  typedef BagChunk<FP8> C;
  typedef typename C::Q Q;
  constexpr int D = 64, U = C::kU;
  constexpr int ROWB = 2048;                      // the output row (<= 1024 columns)
  constexpr int WAVEB = ROWB + kBagStage * 12;    // + staged rows (int64) + staged weights (fp32)
  __shared__ __attribute__((aligned(16))) uint8_t lds[4 * WAVEB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * (blockDim.x / 64) + w;
  if (b >= B) return;
  const int r = lane & 31, h = lane >> 5;
  const int nv = T + 1;
  bf16* o = reinterpret_cast<bf16*>(lds + w * WAVEB);
  int64_t* srow = reinterpret_cast<int64_t*>(lds + w * WAVEB + ROWB);
  float* sw = reinterpret_cast<float*>(lds + w * WAVEB + ROWB + kBagStage * 8);
  // the dense row's chunk lane & 7 (lanes 8.. repeat the same 128 bytes: no branch around the load)
  const bf16x8 dv = *reinterpret_cast<const bf16x8*>(dense + int64_t(b) * ldd + (lane & 7) * 8);

  // 1. stage (row, weight) of the candidate's T * hot ids
  const int n = T * hot;
  ArenaRow ar{nullptr, nullptr, false, kArenaAllWeights, 4};
  if (arena) ar = arena_row(arena, kArenaPayloadOff, b);
  for (int e = lane; e < n; e += 64) {
    const int t = e / hot;
    int64_t id = 0;
    float wv = 1.f;
    if (arena) {  // padding rows: id 0, weight 0 (what the unpack pass leaves for them)
      wv = 0.f;
      if (ar.ids) arena_feature(ar, id_col0 + e, id, wv);
    } else {
      id = int64_t(ids[int64_t(b) * ldi + e]);
      if (wts) wv = wts[int64_t(b) * ldw + e];
    }
    const int64_t v = bag_mod(id, modulo_f[t]);
    srow[e] = min(max(offset_f[t] + v, int64_t(0)), table_rows - 1);
    sw[e] = wv;
  }
  if (lane < D / 8) *reinterpret_cast<bf16x8*>(o + lane * 8) = dv;  // the row's first 64 columns
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // 2. pool this lane's table: K positions 16 s + 8 h .. + 8 of every k-step s
  const bool has_row = r >= 1 && r < nv;
  const int e0 = has_row ? (r - 1) * hot : 0;
  const float sc = (FP8 && has_row) ? scale[r - 1] : 1.f;
  const uint8_t* base = table + h * C::kHalf;
  float acc[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) acc[i] = 0.f;
  for (int j0 = 0; j0 < hot; j0 += U) {
    Q q[U][4];
    float wu[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = has_row && j0 + u < hot;
      const int e = ok ? e0 + j0 + u : 0;  // entry 0 is always staged; weight 0 masks it
      const uint8_t* src = base + srow[e] * C::kRowBytes;
      wu[u] = ok ? sw[e] : 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) q[u][s] = *reinterpret_cast<const Q*>(src + s * C::kStep);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float v[8];
        C::unpack(q[u][s], sc, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[8 * s + i] = __builtin_fmaf(v[i], wu[u], acc[8 * s + i]);
      }
  }

  // 3. interact: r = 0 takes the dense chunk 2 s + h back from the LDS row (a broadcast read)
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const bf16x8 xd = *reinterpret_cast<const bf16x8*>(o + 16 * s + 8 * h);
    bf16x8 x;
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = f2bf(has_row ? acc[8 * s + i] : 0.f);
    x = r == 0 ? xd : x;
    z = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, x, z, 0, 0, 0);
  }
  // assemble the rest of the row behind the dense columns: [lower triangle | zeros]
  const int n8 = out_cols / 8;
  for (int c = D / 8 + lane; c < n8; c += 64) *reinterpret_cast<bf16x8*>(o + c * 8) = bf16x8{};
  __builtin_amdgcn_wave_barrier();
  const int col = lane & 31;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int rowi = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
    if (rowi < nv && col < rowi) o[D + rowi * (rowi - 1) / 2 + col] = f2bf(z[reg]);
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  bf16* dst = out + int64_t(b) * ldo;
  for (int c = lane; c < n8; c += 64) *reinterpret_cast<bf16x8*>(dst + c * 8) = *reinterpret_cast<const bf16x8*>(o + c * 8);
}

template <typename IdT>
__global__ void __launch_bounds__(256) dot_interact_bag_kernel(
    const bf16* __restrict__ dense, int64_t ldd, const bf16* __restrict__ table, int64_t table_rows,
    const IdT* __restrict__ ids, int64_t ldi, const float* __restrict__ wts, int64_t ldw, int hot,
    const int64_t* __restrict__ modulo_f, const int64_t* __restrict__ offset_f, int T, int B, bf16* __restrict__ out,
    int64_t ldo, int out_cols, const uint8_t* __restrict__ arena, int id_col0) {
  dot_interact_bag_body<false, IdT>(dense, ldd, reinterpret_cast<const uint8_t*>(table), table_rows, nullptr, ids, ldi,
                                    wts, ldw, hot, modulo_f, offset_f, T, B, out, ldo, out_cols, arena, id_col0);
}

template <typename IdT>
__global__ void __launch_bounds__(256) dot_interact_bag_fp8_kernel(
    const bf16* __restrict__ dense, int64_t ldd, const uint8_t* __restrict__ codes, int64_t table_rows,
    const float* __restrict__ scale, const IdT* __restrict__ ids, int64_t ldi, const float* __restrict__ wts,
    int64_t ldw, int hot, const int64_t* __restrict__ modulo_f, const int64_t* __restrict__ offset_f, int T, int B,
    bf16* __restrict__ out, int64_t ldo, int out_cols, const uint8_t* __restrict__ arena, int id_col0) {
  dot_interact_bag_body<true, IdT>(dense, ldd, codes, table_rows, scale, ids, ldi, wts, ldw, hot, modulo_f, offset_f, T,
                                   B, out, ldo, out_cols, arena, id_col0);
}

}  // namespace kern

using namespace kern;

// the limits both launchers share (file header); align = the table's load width
static bool bag_args_ok(const void* dense, int64_t ldd, const void* table, int64_t table_rows, int align,
                        const void* ids, int64_t ldi, const float* wts, int64_t ldw, int hot,
                        const int64_t* modulo_f, const int64_t* offset_f, int T, int B, const void* out, int64_t ldo,
                        int out_cols, const void* arena, int id_col0) {
  if (B < 0 || T < 1 || T + 1 > 32 || hot < 2 || int64_t(T) * hot > kBagStage) return false;
  const int64_t n = int64_t(T) * hot;
  if (out_cols % 8 || out_cols > 1024 || out_cols < 64 + (T + 1) * T / 2 || ldo % 8 || ldo < out_cols) return false;
  if (ldd % 8 || ldd < 64 || table_rows < 1 || !dense || !table || !modulo_f || !offset_f || !out) return false;
  if (arena ? id_col0 < 0 : (!ids || ldi < n || (wts && ldw < n))) return false;
  return reinterpret_cast<uintptr_t>(table) % align == 0 && reinterpret_cast<uintptr_t>(dense) % 16 == 0 &&
         reinterpret_cast<uintptr_t>(out) % 16 == 0;
}

hipError_t launch_dot_interaction_bag(const void* dense, int64_t ldd, const void* table, int64_t table_rows,
                                      const void* ids, bool ids64, int64_t ldi, const float* wts, int64_t ldw, int hot,
                                      const int64_t* modulo_f, const int64_t* offset_f, int T, int B, void* out,
                                      int64_t ldo, int out_cols, hipStream_t st, const void* arena, int id_col0) {
  if (B == 0) return hipSuccess;
  if (!bag_args_ok(dense, ldd, table, table_rows, 16, ids, ldi, wts, ldw, hot, modulo_f, offset_f, T, B, out, ldo,
                   out_cols, arena, id_col0))
    return hipErrorInvalidValue;
  const uint8_t* ar = static_cast<const uint8_t*>(arena);
  dim3 grid((B + 3) / 4), block(256);
  if (ids64)
    hipLaunchKernelGGL(dot_interact_bag_kernel<int64_t>, grid, block, 0, st, static_cast<const bf16*>(dense), ldd,
                       static_cast<const bf16*>(table), table_rows, static_cast<const int64_t*>(ids), ldi, wts, ldw,
                       hot, modulo_f, offset_f, T, B, static_cast<bf16*>(out), ldo, out_cols, ar, id_col0);
  else
    hipLaunchKernelGGL(dot_interact_bag_kernel<int32_t>, grid, block, 0, st, static_cast<const bf16*>(dense), ldd,
                       static_cast<const bf16*>(table), table_rows, static_cast<const int32_t*>(ids), ldi, wts, ldw,
                       hot, modulo_f, offset_f, T, B, static_cast<bf16*>(out), ldo, out_cols, ar, id_col0);
  return hipGetLastError();
}

hipError_t launch_dot_interaction_bag_fp8(const void* dense, int64_t ldd, const void* codes, int64_t table_rows,
                                          const float* scale, const void* ids, bool ids64, int64_t ldi,
                                          const float* wts, int64_t ldw, int hot, const int64_t* modulo_f,
                                          const int64_t* offset_f, int T, int B, void* out, int64_t ldo, int out_cols,
                                          hipStream_t st, const void* arena, int id_col0) {
  if (B == 0) return hipSuccess;
  if (!scale || !bag_args_ok(dense, ldd, codes, table_rows, 8, ids, ldi, wts, ldw, hot, modulo_f, offset_f, T, B, out,
                             ldo, out_cols, arena, id_col0))
    return hipErrorInvalidValue;
  const uint8_t* ar = static_cast<const uint8_t*>(arena);
  const uint8_t* c = static_cast<const uint8_t*>(codes);
  dim3 grid((B + 3) / 4), block(256);
  if (ids64)
    hipLaunchKernelGGL(dot_interact_bag_fp8_kernel<int64_t>, grid, block, 0, st, static_cast<const bf16*>(dense), ldd, c,
                       table_rows, scale, static_cast<const int64_t*>(ids), ldi, wts, ldw, hot, modulo_f, offset_f, T,
                       B, static_cast<bf16*>(out), ldo, out_cols, ar, id_col0);
  else
    hipLaunchKernelGGL(dot_interact_bag_fp8_kernel<int32_t>, grid, block, 0, st, static_cast<const bf16*>(dense), ldd, c,
                       table_rows, scale, static_cast<const int32_t*>(ids), ldi, wts, ldw, hot, modulo_f, offset_f, T,
                       B, static_cast<bf16*>(out), ldo, out_cols, ar, id_col0);
  return hipGetLastError();
}

}  // namespace dtfs
