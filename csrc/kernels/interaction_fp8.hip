// DLRM lookups from fp8 embedding tables (ModelConfig.table_dtype: fp8).
//
// Storage: codes e4m3 (OCP) [T * rows][64], one row = 64 bytes (two rows per
// 128-byte line), and one fp32 scale per table that is an exact power of two:
//   value(t, r, c) = float(codes[offset_f[t] + r][c]) * scale[t]
// Every e4m3 value times a power of two is exactly a bf16 value, so the
// kernels below compute bit for bit what their bf16 twins (interaction.hip
// dot_interact_gather_kernel, embedding.hip bag_kernel) compute on the
// dequantised table, from half the bytes per random row read.
#include "common.h"
#include "fp8_rows.h"
#include "launchers.h"

namespace dtfs {
namespace kern {

// K1 + K5 on fp8 tables: dot_interact_gather_kernel (interaction.hip) with the
// T rows of a candidate read as e4m3 codes. One wave per candidate, lane
// (r, h): r = 0 holds the dense vector, r = 1..T the row of table r - 1. For
// k-step s the lane owns K positions 16 s + 8 h .. + 8 - the bf16 kernel's
// operand order - which are the 8 code bytes at byte 16 s + 8 h of its row:
// four 8-byte loads per lane, all issued before the first MFMA (2 KB of
// independent random reads in flight per wave). Codes -> bf16 in registers,
// then the same four v_mfma_f32_32x32x16_bf16 and the same LDS-assembled
// [dense | lower triangle | zero pad] row written as 16-byte vectors.
//
// Every load is unconditional. Written as `if (r == 0) dense load else code
// load`, the two load widths land in divergent blocks whose other side zeroes
// the destination, and the compiler waits for each code load before it issues
// the next (vmcnt(1) after every pair: one random read in flight, not four).
// So lanes without a table row read row 0 (always there) and are masked after
// the load, and the dense vector goes through the wave's LDS row, where the
// output needs it anyway: lanes 0..7 load its eight 16-byte chunks once
// (the bf16 kernel reads it twice), and every lane reads chunk 2 s + h back as
// the r = 0 operand of k-step s (a broadcast ds_read_b128; only r = 0 keeps it).
template <typename IdT>
__global__ void __launch_bounds__(256) dot_interact_gather_fp8_kernel(
    const bf16* __restrict__ dense, int64_t ldd, const uint8_t* __restrict__ codes, int64_t table_rows,
    const float* __restrict__ scale, const IdT* __restrict__ ids, int64_t ldi, const int64_t* __restrict__ modulo_f,
    const int64_t* __restrict__ offset_f, int T, int B, bf16* __restrict__ out, int64_t ldo, int out_cols,
    const uint8_t* __restrict__ arena, int id_col0) {
  constexpr int D = 64;
  constexpr int ROWB = 4 * 2048;  // LDS bytes per block: 4 waves x one output row (<= 1024 columns)
  __shared__ __attribute__((aligned(16))) uint8_t lds[ROWB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * (blockDim.x / 64) + w;
  if (b >= B) return;
  const int r = lane & 31, h = lane >> 5;
  const int nv = T + 1;
  // the dense row's chunk lane & 7 (lanes 8.. repeat the same 128 bytes: no branch around the load)
  const bf16x8 dv = *reinterpret_cast<const bf16x8*>(dense + int64_t(b) * ldd + (lane & 7) * 8);
  const bool has_row = r >= 1 && r < nv;
  const uint8_t* src = codes;
  float sc = 1.f;
  if (has_row) {
    const int t = r - 1;
    const int64_t m = modulo_f[t];
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
    src = codes + min(max(offset_f[t] + v, int64_t(0)), table_rows - 1) * D;
    sc = scale[t];
  }
  uint2 q[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) q[s] = *reinterpret_cast<const uint2*>(src + 16 * s + 8 * h);
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

// K1b on fp8 tables: bag_kernel<64> (embedding.hip) reading 8 code bytes where
// it reads 8 bf16. One wave per bag, lane (sub, dl): 8 index slots x 8 lanes
// of 8 dims. Bag b belongs to table b % T (the [B, T] bag layout DLRM.lookup
// builds) and takes that table's scale: acc += (float(code) * scale) * w.
template <typename IdT>
__global__ void __launch_bounds__(256) bag_fp8_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ scale,
                                                      int T, const IdT* __restrict__ idx,
                                                      const int64_t* __restrict__ offsets, const float* __restrict__ psw,
                                                      int nbags, int64_t nnz, int64_t modulo, int mean,
                                                      float* __restrict__ out_f32, bf16* __restrict__ out_bf16,
                                                      int64_t out_stride) {
  constexpr int D = 64;
  constexpr int LPR = D / 8;
  constexpr int BPW = kWave / LPR;  // index slots per wave pass
  const int lane = threadIdx.x & 63;
  const int bag = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (bag >= nbags) return;
  const int sub = lane / LPR, dl = (lane % LPR) * 8;
  const float s = scale[bag % T];
  // clamp the CSR range so a malformed request can never read out of bounds
  const int64_t beg = min(max(offsets[bag], int64_t(0)), nnz);
  const int64_t end = min(max(offsets[bag + 1], beg), nnz);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int64_t i = beg + sub; i < end; i += BPW) {
    const int64_t r = hash_row(int64_t(idx[i]), modulo);
    const float w = psw ? psw[i] : 1.f;
    const uint2 q = *reinterpret_cast<const uint2*>(codes + r * D + dl);
    const f32x2 v[4] = {__builtin_amdgcn_cvt_pk_f32_fp8(int(q.x), false), __builtin_amdgcn_cvt_pk_f32_fp8(int(q.x), true),
                        __builtin_amdgcn_cvt_pk_f32_fp8(int(q.y), false), __builtin_amdgcn_cvt_pk_f32_fp8(int(q.y), true)};
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += (v[j >> 1][j & 1] * s) * w;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int o = LPR; o < kWave; o <<= 1) acc[j] += __shfl_xor(acc[j], o, 64);
  if (sub != 0) return;
  const float sc = (mean && end > beg) ? 1.f / float(end - beg) : 1.f;
  if (out_f32) {
    float4* p = reinterpret_cast<float4*>(out_f32 + int64_t(bag) * out_stride + dl);
    p[0] = make_float4(acc[0] * sc, acc[1] * sc, acc[2] * sc, acc[3] * sc);
    p[1] = make_float4(acc[4] * sc, acc[5] * sc, acc[6] * sc, acc[7] * sc);
  } else {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(acc[j] * sc);
    *reinterpret_cast<bf16x8*>(out_bf16 + int64_t(bag) * out_stride + dl) = o;
  }
}

}  // namespace kern

using namespace kern;

hipError_t launch_dot_interaction_gather_fp8(const void* dense, int64_t ldd, const void* codes, int64_t table_rows,
                                             const float* scale, const void* ids, bool ids64, int64_t ldi,
                                             const int64_t* modulo_f, const int64_t* offset_f, int T, int B, void* out,
                                             int64_t ldo, int out_cols, hipStream_t st, const void* arena,
                                             int id_col0) {
  if (B == 0) return hipSuccess;
  if (B < 0 || T < 1 || T + 1 > 32 || out_cols % 8 || out_cols > 1024 || out_cols < 64 + (T + 1) * T / 2 || ldo % 8 ||
      ldo < out_cols || ldd % 8 || ldd < 64 || (!arena && (!ids || ldi < T)) || (arena && id_col0 < 0) ||
      table_rows < 1 || !dense || !codes || !scale || !modulo_f || !offset_f || !out ||
      reinterpret_cast<uintptr_t>(codes) % 8 || reinterpret_cast<uintptr_t>(dense) % 16 ||
      reinterpret_cast<uintptr_t>(out) % 16)
    return hipErrorInvalidValue;
  const uint8_t* ar = static_cast<const uint8_t*>(arena);
  dim3 grid((B + 3) / 4), block(256);
  if (ids64)
    hipLaunchKernelGGL(dot_interact_gather_fp8_kernel<int64_t>, grid, block, 0, st, static_cast<const bf16*>(dense),
                       ldd, static_cast<const uint8_t*>(codes), table_rows, scale, static_cast<const int64_t*>(ids),
                       ldi, modulo_f, offset_f, T, B, static_cast<bf16*>(out), ldo, out_cols, ar, id_col0);
  else
    hipLaunchKernelGGL(dot_interact_gather_fp8_kernel<int32_t>, grid, block, 0, st, static_cast<const bf16*>(dense),
                       ldd, static_cast<const uint8_t*>(codes), table_rows, scale, static_cast<const int32_t*>(ids),
                       ldi, modulo_f, offset_f, T, B, static_cast<bf16*>(out), ldo, out_cols, ar, id_col0);
  return hipGetLastError();
}

hipError_t launch_embedding_bag_fp8(const void* codes, int64_t table_rows, const float* scale, int T, const void* idx,
                                    bool idx64, const int64_t* offsets, const float* psw, int nbags, int64_t nnz,
                                    int64_t modulo, bool mean, float* out_f32, void* out_bf16, int64_t out_stride,
                                    hipStream_t st) {
  if (nbags == 0) return hipSuccess;
  if (nbags < 0 || nnz < 0 || T < 1 || !codes || !scale || !offsets || (nnz > 0 && !idx) || modulo < 1 ||
      modulo > table_rows || (out_f32 == nullptr) == (out_bf16 == nullptr) || out_stride < 64 || out_stride % 8 ||
      reinterpret_cast<uintptr_t>(codes) % 8)
    return hipErrorInvalidValue;
  const uint8_t* c = static_cast<const uint8_t*>(codes);
  bf16* ob = static_cast<bf16*>(out_bf16);
  dim3 grid((nbags + 3) / 4), block(256);
  if (idx64)
    hipLaunchKernelGGL(bag_fp8_kernel<int64_t>, grid, block, 0, st, c, scale, T, static_cast<const int64_t*>(idx), offsets,
                       psw, nbags, nnz, modulo, int(mean), out_f32, ob, out_stride);
  else
    hipLaunchKernelGGL(bag_fp8_kernel<int32_t>, grid, block, 0, st, c, scale, T, static_cast<const int32_t*>(idx), offsets,
                       psw, nbags, nnz, modulo, int(mean), out_f32, ob, out_stride);
  return hipGetLastError();
}

}  // namespace dtfs
