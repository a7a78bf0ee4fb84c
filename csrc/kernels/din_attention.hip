// DIN (Deep Interest Network) target attention over the behaviour history, one
// launch from ids / weights / table to the MLP input x [B, (P + 2) 64].
//
// Request row: columns 0 .. P-1 profile fields, column P the candidate item,
// columns P+1 .. P+H the history. For one candidate, D = 64:
//   e_f  = bf16(fp32(w_f) * row(id_f mod V))              every field
//   q    = e_P ;  k_h = e_{P+1+h}
//   p_h  = bf16(q * k_h)                                   fp32 product, one rounding
//   z1_h = Wq q + Wk k_h + Wp p_h + b1                     fp32            [a1]
//   a1_h = bf16(prelu(z1_h, alpha1))
//   a2_h = prelu(W2 a1_h + b2, alpha2)                     fp32            [a2]
//   s_h  = w3 . a2_h + b3                                  fp32, no softmax
//   v    = bf16(sum_h s_h k_h)                             fp32
//   x    = [e_0 | .. | e_{P-1} | q | v]
// The fp32 sums run in the MFMA's order and, for v, over the four 16-row blocks
// inside a lane and then over the 16 lanes of a block: not h ascending. No
// rounding is added to the contract (s_h stays fp32: the pooling is VALU work).
//
// Work split: 512-thread workgroups, one per CU at most (grid-stride over the
// candidates), one wave per candidate at a time. The MFMA M dimension is the
// history position: NMB = ceil(H / 16) blocks of 16 rows (template parameter),
// v_mfma_f32_16x16x32_bf16 as D = W_frag x A_frag^T, lane (fr, fq) = (lane & 15,
// lane >> 4) holding C[m = fr][n = 4 fq .. + 3].
//
//   * Lane (fr, fq) loads, for every block mb, the two 16-byte pieces
//     32 kc + 8 fq .. + 8 (kc = 0, 1) of history row 16 mb + fr straight from
//     the table: after the weight scaling these 2 NMB registers quads ARE the A
//     fragments of the Wk product, the source of p_h (multiplied by the lane's
//     piece of q, which every lane loads from the candidate's row) and the
//     operands of the pooling. A table row is read from HBM once; nothing of
//     size H goes through LDS but the 16-lane reduction of v.
//   * Layer 1 is [16 NMB, 128] x [128, a1p], k and p side by side on K, in
//     pairs of 16-unit blocks. The accumulators start from Wq q + b1, which is
//     two more MFMAs per block on an A operand whose 16 rows are all q (the
//     lane's q pieces as they are): the row-broadcast term costs no shuffle.
//   * The host permutes the a1 units inside every group of 32 (block t,
//     fragment row 4 j + s = unit 8 j + 4 t + s, as cross_mix.hip does for U),
//     so a lane's 2 x 4 outputs of a pair are 8 consecutive units of its row:
//     prelu, bf16, and the pair is layer 2's A fragment of K chunk `pair`
//     without leaving the registers. Layer 2 accumulates [16 NMB, a2p] over
//     the pairs; prelu, the w3 dot and the sum over fq (two shuffles) give s_h
//     for row 16 mb + fr in every lane of that row.
//   * Pooling: lane partials sum_mb s k over its 16 columns, 16 x 68 fp32 per
//     wave in LDS, lane d sums column d over the 16 rows and writes v_d.
//   * Ids and weights are read in place (row-strided, int32 / int64 ids), one
//     column per lane, one candidate ahead; the lane that reads an id hashes it
//     (32-bit fast path, 64-bit modulo) and leaves the table row and weight in
//     the wave's LDS slice. Profile columns and the candidate are taken in
//     reverse (entry j = column P - j, 64 entries per chunk), so entry 0 is q;
//     they are copied through to x 8 rows per wave instruction, 4 instructions
//     in flight. Every load is unconditional: lanes and blocks past H or P read
//     a staged entry with weight 0, and s_h is forced to 0 past H.
//   * a1 / a2 are zero padded to a1p (multiple of 32) / a2p (multiple of 16) by
//     ops.din_attention_pack. The packed weights (fragment order, <= 64 KB) and
//     the fp32 vectors are copied to LDS once per workgroup and stay there.
//
// LDS map (bytes): [0, 65536) W1 = [Wk | Wp] frags (a1p x 128), Wq frags
// (a1p x 64), W2 frags (a2p x a1p), back to back; [65536, 67584) b1, alpha1
// (permuted as the units), b2, alpha2, w3, b3; then 5376 per wave: front rows /
// weights (64 + 64), history rows / weights (64 + 64), the pooling tile.
// 110592 in all: one workgroup (8 waves, 2 per SIMD) per CU.
//
// Registers per lane (int64 ids; int32 two fewer): 114 / 151 / 185 / 222 VGPRs
// at NMB = 1 / 2 / 3 / 4, no AGPRs, no scratch; 2 waves per SIMD (the LDS, one
// workgroup per CU, sets that; the registers allow it). Left to the compiler,
// p_h is hoisted out of the pair loop (8 NMB more registers) and NMB = 4
// spills: q is made opaque per pair and the K chunks are fenced off from each
// other. Limits (launcher): D = 64, 1 <= H <= 64, a1p <= 128, a2p <= 64,
// P >= 0, V < 2^31, out rows 16-byte aligned with ldo % 8 == 0.
#include <algorithm>

#include "common.h"
#include "launchers.h"

namespace dtfs {
namespace kern {

namespace {
constexpr int kDinWBytes = 65536, kDinFBytes = 2048, kDinWaves = 8;
constexpr int kDinPartLd = 68;                               // fp32 per pooling-tile row (16-byte rows, 4 banks apart)
constexpr int kDinWaveBytes = 4 * 64 * 4 + 16 * kDinPartLd * 4;

// id -> python-style non-negative id mod m (interaction_bag.hip's bag_mod)
__device__ __forceinline__ int din_mod(int64_t id, int64_t m) {
  if (((uint64_t(id) | uint64_t(m)) >> 32) == 0) return int(uint32_t(id) % uint32_t(m));
  const int64_t v = id % m;
  return int(v < 0 ? v + m : v);
}

// bf16(w * x) of 8 packed bf16 values
__device__ __forceinline__ bf16x8 din_scale(const uint4& q, float w) {
  const uint32_t d[4] = {q.x, q.y, q.z, q.w};
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[2 * i] = f2bf(__uint_as_float(d[i] << 16) * w);
    o[2 * i + 1] = f2bf(__uint_as_float(d[i] & 0xffff0000u) * w);
  }
  return o;
}

__device__ __forceinline__ float din_prelu(float x, float a) { return x > 0.f ? x : a * x; }

__device__ __forceinline__ void din_lds_fence() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
}  // namespace

template <int NMB, typename IdT>
__global__ void __launch_bounds__(512)
    din_attention_kernel(const bf16* __restrict__ table, int64_t V, const IdT* __restrict__ ids, int64_t ldi,
                         const float* __restrict__ wts, int64_t ldw, int B, int P, int H, int a1p, int a2p,
                         const uint4* __restrict__ wpack, const float* __restrict__ fpack, bf16* __restrict__ out,
                         int64_t ldo) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kDinWBytes + kDinFBytes + kDinWaves * kDinWaveBytes];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int NP = a1p / 32, NB2 = a2p / 16;

  // the packed weights and vectors, once per workgroup
  {
    uint4* wl = reinterpret_cast<uint4*>(lds);
    const int n16 = (a1p * 192 + a2p * a1p) / 8;  // 16-byte pieces (<= 4096)
    for (int i = threadIdx.x; i < n16; i += 512) wl[i] = wpack[i];
    float* fl = reinterpret_cast<float*>(lds + kDinWBytes);
    const int nf = 2 * a1p + 3 * a2p + 1;  // <= 449
    for (int i = threadIdx.x; i < nf; i += 512) fl[i] = fpack[i];
  }
  __syncthreads();
  const bf16x8* W1F = reinterpret_cast<const bf16x8*>(lds) + lane;  // frag (nb, kc): (4 nb + kc) * 64
  const bf16x8* WqF = W1F + a1p * 16;                               // frag (nb, kc): (2 nb + kc) * 64
  const bf16x8* W2F = WqF + a1p * 8;                                // frag (nb2, pr): (NP nb2 + pr) * 64
  const float* fb1 = reinterpret_cast<const float*>(lds + kDinWBytes);
  const float* fal1 = fb1 + a1p;
  const float* fb2 = fal1 + a1p;
  const float* fal2 = fb2 + a2p;
  const float* fw3 = fal2 + a2p;
  const float b3 = fw3[a2p];

  uint8_t* wl = lds + kDinWBytes + kDinFBytes + wid * kDinWaveBytes;
  int* srowF = reinterpret_cast<int*>(wl);
  float* swF = reinterpret_cast<float*>(wl + 256);
  int* srowH = reinterpret_cast<int*>(wl + 512);
  float* swH = reinterpret_cast<float*>(wl + 768);
  float* part = reinterpret_cast<float*>(wl + 1024);

  const int step = gridDim.x * kDinWaves;
  int b = blockIdx.x * kDinWaves + wid;
  if (b >= B) return;

  // this lane's two columns of a candidate: front entry `lane` (column P - lane)
  // and history position `lane`; lanes past P / H repeat a column with weight 0
  const int cF = P - min(lane, P), cH = P + 1 + min(lane, H - 1);
  const bool okF = lane <= P, okH = lane < H;
  auto fetch = [&](int bb, int64_t& iF, float& wF, int64_t& iH, float& wH) {
    const IdT* ip = ids + int64_t(bb) * ldi;
    const float* wp = wts + int64_t(bb) * ldw;
    iF = int64_t(ip[cF]);
    iH = int64_t(ip[cH]);
    wF = wp[cF];
    wH = wp[cH];
  };
  // 8 front rows per wave instruction, 4 instructions in flight: entry
  // j0 + 8 u + (lane >> 3) -> x columns (P - entry) 64 .. + 64
  const int sub = lane >> 3, piece = (lane & 7) * 8;
  auto copy_front = [&](int bb, int j0) {
    const int n = min(P + 1 - j0, 64);
    bf16* orow = out + int64_t(bb) * ldo + piece;
    for (int r0 = 0; r0 < n; r0 += 32) {
      uint4 raw[4];
      float w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int jj = r0 + 8 * u + sub;  // <= 63: every entry of the chunk is staged
        w[u] = swF[jj];
        raw[u] = *reinterpret_cast<const uint4*>(table + int64_t(srowF[jj]) * 64 + piece);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + r0 + 8 * u + sub;
        if (j <= P) *reinterpret_cast<bf16x8*>(orow + int64_t(P - j) * 64) = din_scale(raw[u], w[u]);
      }
    }
  };

  int64_t iF, iH;
  float wF, wH;
  fetch(b, iF, wF, iH, wH);
  for (; b < B; b += step) {
    // stage this candidate's rows and weights, then fetch the next candidate's columns
    srowF[lane] = din_mod(iF, V);
    swF[lane] = okF ? wF : 0.f;
    srowH[lane] = din_mod(iH, V);
    swH[lane] = okH ? wH : 0.f;
    fetch(min(b + step, B - 1), iF, wF, iH, wH);
    din_lds_fence();

    // history rows and q, straight into the MFMA A layout
    uint4 rawq[2], rawk[NMB][2];
    float wk[NMB];
    const float wq = swF[0];
    {
      const bf16* qrow = table + int64_t(srowF[0]) * 64 + 8 * fq;
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) rawq[kc] = *reinterpret_cast<const uint4*>(qrow + 32 * kc);
#pragma unroll
      for (int mb = 0; mb < NMB; ++mb) {
        const bf16* krow = table + int64_t(srowH[16 * mb + fr]) * 64 + 8 * fq;
        wk[mb] = swH[16 * mb + fr];
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) rawk[mb][kc] = *reinterpret_cast<const uint4*>(krow + 32 * kc);
      }
    }
    // profile fields and q -> x (entries past the first 64: staged here, chunk by chunk)
    copy_front(b, 0);
    for (int j0 = 64; j0 <= P; j0 += 64) {
      const int j = j0 + lane, c = P - min(j, P);
      const int row = din_mod(int64_t(ids[int64_t(b) * ldi + c]), V);
      const float w = j <= P ? wts[int64_t(b) * ldw + c] : 0.f;
      din_lds_fence();
      srowF[lane] = row;
      swF[lane] = w;
      din_lds_fence();
      copy_front(b, j0);
    }

    bf16x8 qf[2], kf[NMB][2];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      qf[kc] = din_scale(rawq[kc], wq);
#pragma unroll
      for (int mb = 0; mb < NMB; ++mb) kf[mb][kc] = din_scale(rawk[mb][kc], wk[mb]);
    }

    // layer 2 accumulators start from b2
    f32x4 acc2[NMB][4];
#pragma unroll
    for (int nb2 = 0; nb2 < 4; ++nb2) {
      const f32x4 bv = nb2 < NB2 ? *reinterpret_cast<const f32x4*>(fb2 + 16 * nb2 + 4 * fq) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int mb = 0; mb < NMB; ++mb) acc2[mb][nb2] = bv;
    }

    for (int pr = 0; pr < NP; ++pr) {
      // (q opaque per pair: p_h is recomputed here, 4 registers, instead of 8 NMB hoisted out of the loop)
      asm volatile("" : "+v"(qf[0]), "+v"(qf[1]));
      // layer 1, units 32 pr .. + 32 (two blocks): start from Wq q + b1
      f32x4 acc1[2][NMB];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int nb = 2 * pr + t;
        f32x4 a = *reinterpret_cast<const f32x4*>(fb1 + 16 * nb + 4 * fq);
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WqF[(2 * nb + kc) * 64], qf[kc], a, 0, 0, 0);
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) acc1[t][mb] = a;
      }
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        __builtin_amdgcn_sched_barrier(0);  // keep the fragment reads of later K chunks out of this one's registers
        bf16x8 wf[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) wf[t] = W1F[(4 * (2 * pr + t) + kc) * 64];
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) {
          bf16x8 af = kf[mb][kc & 1];
          if (kc >= 2) {  // p = bf16(q * k)
#pragma unroll
            for (int e = 0; e < 8; ++e) af[e] = f2bf(bf2f(qf[kc & 1][e]) * bf2f(af[e]));
          }
#pragma unroll
          for (int t = 0; t < 2; ++t) acc1[t][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t], af, acc1[t][mb], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      // prelu, bf16: the pair is layer 2's A fragment of K chunk pr
      f32x4 al[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) al[t] = *reinterpret_cast<const f32x4*>(fal1 + 16 * (2 * pr + t) + 4 * fq);
      bf16x8 w2f[4];
#pragma unroll
      for (int nb2 = 0; nb2 < 4; ++nb2) w2f[nb2] = W2F[(NP * min(nb2, NB2 - 1) + pr) * 64];
#pragma unroll
      for (int mb = 0; mb < NMB; ++mb) {
        bf16x8 a1f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) a1f[4 * t + i] = f2bf(din_prelu(acc1[t][mb][i], al[t][i]));
#pragma unroll
        for (int nb2 = 0; nb2 < 4; ++nb2)
          if (nb2 < NB2) acc2[mb][nb2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2f[nb2], a1f, acc2[mb][nb2], 0, 0, 0);
      }
    }

    // s_h = w3 . prelu(a2) + b3 for row 16 mb + fr (0 past H)
    float s[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb) s[mb] = 0.f;
#pragma unroll
    for (int nb2 = 0; nb2 < 4; ++nb2) {
      if (nb2 >= NB2) continue;
      const f32x4 al2 = *reinterpret_cast<const f32x4*>(fal2 + 16 * nb2 + 4 * fq);
      const f32x4 w3 = *reinterpret_cast<const f32x4*>(fw3 + 16 * nb2 + 4 * fq);
#pragma unroll
      for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
        for (int i = 0; i < 4; ++i) s[mb] = __builtin_fmaf(din_prelu(acc2[mb][nb2][i], al2[i]), w3[i], s[mb]);
    }
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb) {
      float v = s[mb];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      s[mb] = 16 * mb + fr < H ? v + b3 : 0.f;
    }

    // v = bf16(sum_h s_h k_h): lane partials over its blocks, then over the 16 rows through LDS
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      float pv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) pv[e] = 0.f;
#pragma unroll
      for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
        for (int e = 0; e < 8; ++e) pv[e] = __builtin_fmaf(s[mb], bf2f(kf[mb][kc][e]), pv[e]);
      float* dst = part + fr * kDinPartLd + 32 * kc + 8 * fq;
      *reinterpret_cast<f32x4*>(dst) = f32x4{pv[0], pv[1], pv[2], pv[3]};
      *reinterpret_cast<f32x4*>(dst + 4) = f32x4{pv[4], pv[5], pv[6], pv[7]};
    }
    din_lds_fence();
    float vs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) vs += part[r * kDinPartLd + lane];
    out[int64_t(b) * ldo + int64_t(P + 1) * 64 + lane] = f2bf(vs);
    din_lds_fence();  // the next candidate's staging and pooling tile
  }
}

}  // namespace kern

using namespace kern;

hipError_t launch_din_attention(const void* table, int64_t V, const void* ids, bool ids64, int64_t ldi,
                                const float* wts, int64_t ldw, int B, int P, int H, int a1p, int a2p,
                                const void* wpack, const float* fpack, void* out, int64_t ldo, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (B < 0 || P < 0 || H < 1 || H > 64 || a1p < 32 || a1p > 128 || a1p % 32 || a2p < 16 || a2p > 64 || a2p % 16 ||
      V < 1 || V >= (int64_t(1) << 31))
    return hipErrorInvalidValue;
  const int64_t F = int64_t(P) + 1 + H;
  if (!table || !ids || !wts || !wpack || !fpack || !out || ldi < F || ldw < F || ldo % 8 || ldo < (int64_t(P) + 2) * 64)
    return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(table) % 16 || reinterpret_cast<uintptr_t>(out) % 16 ||
      reinterpret_cast<uintptr_t>(wpack) % 16)
    return hipErrorInvalidValue;
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
      n = 256;
    cus = n;
  }
  const int blocks = std::min((B + kDinWaves - 1) / kDinWaves, cus);
#define DTFS_DIN(N, T)                                                                                            \
  hipLaunchKernelGGL((din_attention_kernel<N, T>), dim3(blocks), dim3(512), 0, st, static_cast<const bf16*>(table), \
                     V, static_cast<const T*>(ids), ldi, wts, ldw, B, P, H, a1p, a2p,                               \
                     static_cast<const uint4*>(wpack), fpack, static_cast<bf16*>(out), ldo)
#define DTFS_DIN_IDS(N) \
  if (ids64)            \
    DTFS_DIN(N, int64_t); \
  else                  \
    DTFS_DIN(N, int32_t)
  switch ((H + 15) / 16) {
    case 1: DTFS_DIN_IDS(1); break;
    case 2: DTFS_DIN_IDS(2); break;
    case 3: DTFS_DIN_IDS(3); break;
    default: DTFS_DIN_IDS(4); break;
  }
#undef DTFS_DIN_IDS
#undef DTFS_DIN
  return hipGetLastError();
}

}  // namespace dtfs
