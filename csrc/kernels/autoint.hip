// AutoInt (Song et al. 2019) interacting layers: multi-head self-attention over
// the F feature fields of one candidate, a whole stack of L layers in ONE
// launch. For one candidate, x [F, 64] bf16, heads in {1, 2, 4}, d = 64 / heads,
// Wq, Wk, Wv, Wres [64 in, 64 out] bf16 per layer, head h owning units h d ..:
//   q, k, v   = bf16(x Wq), bf16(x Wk), bf16(x Wv)       fp32 sums, one rounding each
//   s_h[i, j] = q_h[i] . k_h[j]                          fp32, no 1 / sqrt(d)
//   e_h[i, j] = exp(s_h[i, j] - max_j s_h[i, j])         fp32; keys j >= F: e = 0
//   o_h[i]    = (sum_j bf16(e_h[i, j]) v_h[j]) / sum_j e_h[i, j]
//   y[i]      = bf16(relu(concat_h o_h[i] + x[i] Wres))  the residual product stays fp32
// y is the next layer's x. logit = sum_{f, u} w_out[f, u] float(y^L[f, u]).
// Summation orders: every product sum runs in the MFMA's order; the softmax
// denominator sums a lane's keys 16 kb + 4 fq + i (kb, then i, ascending) and
// then the four fq groups by two butterfly steps; the logit sums a lane's 8-unit
// pieces (row block, then 32-unit chunk, then unit, ascending) in one chain and
// then the 64 lanes by a butterfly: none of them is index ascending. exp is
// v_exp_f32 on (s - max) log2(e); 1 / sum is v_rcp_f32 (1 ulp).
//
// Work split: one wave per candidate, WAVES waves per workgroup, one workgroup
// per CU at most, grid-stride over the candidates. Between loading x and
// storing y^L and the logit nothing of size F x 64 or F x F leaves the
// registers: no LDS, no HBM. NMB = ceil(F / 16) row blocks and the head count
// are template parameters. v_mfma_f32_16x16x32_bf16 throughout: lane (fr, fq) =
// (lane & 15, lane >> 4) supplies A[m = fr][k = 8 fq .. + 7] and
// B[k = 8 fq .. + 7][n = fr] and receives D[m = 4 fq + i][n = fr], i = 0 .. 3.
//
//   * x: lane (fr, fq) loads the 16-byte pieces 32 kc + 8 fq .. + 8 (kc = 0, 1)
//     of row 16 mb + fr. The register quad xf[mb][kc] is the A fragment of x
//     and the B fragment of x^T alike.
//   * Q^T = Wq^T x^T, K^T = Wk^T x^T (weights on A, xf on B): a lane receives 4
//     units of its own row per 16-unit block. The host permutes the output units
//     of all four matrices inside every group of 32 (block t, fragment row
//     4 j + s = unit 8 j + 4 t + s, as cross_mix.hip and din_attention.hip do),
//     so the two blocks of a pair, rounded, are 8 consecutive units 32 g + 8 fq
//     .. + 7 of the row: qf[mb][g] and kf[mb][g] ARE the B fragment of Q^T and
//     the A fragment of K of the score MFMAs.
//   * Scores transposed, S^T = K_h Q_h^T (keys on M, queries on N): a lane holds,
//     for its query 16 qb + fr, the keys 16 kb + 4 fq + i. 1 head: two K chunks;
//     2 heads: chunk h; 4 heads (d = 16): chunk h / 2 with the Q fragment zeroed
//     in the lanes that hold the other head's units (fq / 2 != h % 2): the
//     zero-filled 32-deep chunk, not the 16x16x16 MFMA. Keys >= F get -inf before
//     the max (a zero key would still get exp(0 - max)). Max and sum: in-lane,
//     then two cross-lane steps over fq.
//   * V = x Wv untransposed (xf on A): a lane holds, for unit position fr, the
//     same keys 16 kb + 4 fq + i. Two key blocks, rounded, are the A fragment of
//     V^T for a 32-key chunk, in the key order of the rounded e of the scores
//     (the B fragment of P^T): O^T = V^T P^T needs no transpose. Key blocks past
//     NMB are zero in both.
//   * The O^T accumulators start from Wres^T x^T (same layout as Q^T); the
//     attention part is scaled by 1 / sum e of the lane's query and added. With 4
//     heads a 16-unit block holds units of two heads (the permutation spreads a
//     block over 32 units): its PV product runs once per head and each lane
//     keeps the one of its units' head. relu, bf16, and with the same permutation
//     the pair of blocks is xf[qb][g] of the next layer.
//   * The scores run one (head, query block) at a time: 4 NMB score registers
//     live, not 4 NMB^2 HEADS.
//   * Weights: ops.autoint_pack writes them in fragment order; they are copied to
//     LDS once per workgroup and stay there: 4 x 8 KB per layer, then w_out
//     (fp32, [row block][chunk][lane][8], zero past F, <= 16 KB): 147456 bytes.
//   * Every load is unconditional: rows past F read row F - 1. Such rows are
//     masked as keys, computed as queries (finite duplicates) and never stored;
//     their w_out is zero.
//   * y^L: a lane stores its two 16-byte pieces of row 16 qb + fr; the four fq
//     lanes of a row write 64 contiguous bytes per instruction, and the two
//     instructions of a row block, back to back, complete every 128-byte row.
//   * The next candidate's x is loaded before the current one is computed.
//
// Registers per lane (hipcc, -Rpass-analysis=kernel-resource-usage), heads =
// 1 / 2 / 4, no scratch and no AGPRs unless noted: NMB = 1: 90 / 90 / 90;
// NMB = 2: 166 / 146 / 157; NMB = 3: 200 / 200 / 250; NMB = 4: 250 / 250 and,
// with 4 heads, 256 + 78 AGPRs. All run 512-thread workgroups, 2 waves per SIMD
// (the LDS allows one workgroup per CU), except NMB = 4 with 4 heads: there the
// masked Q fragments and the second PV product per block do not fit 256
// registers (172 bytes of scratch per lane), so that instance runs 256-thread
// workgroups, one wave per SIMD, rather than a split of the query blocks into
// separate passes over K and V. Left to the compiler, the fragment reads of
// later groups are hoisted and NMB = 2 spills: the groups are fenced off.
// Limits (launcher): 1 <= F <= 64, heads in {1, 2, 4}, 1 <= L <= 4, rows of x
// and y 16-byte aligned (base and both strides multiples of 8 elements).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "launchers.h"

namespace dtfs {
namespace kern {

namespace {
constexpr int kAiMatFrags = 8;                       // 16-byte-per-lane fragments of one 64 x 64 matrix: (ub, kc)
constexpr int kAiLayerBytes = 4 * kAiMatFrags * 1024;
constexpr int kAiMaxLayers = 4;
constexpr int kAiOutBytes = 64 * 64 * 4;

__device__ __forceinline__ f32x4 ai_mfma(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
}  // namespace

template <int NMB, int HEADS, int WAVES>
__global__ void __launch_bounds__(64 * WAVES)
    autoint_kernel(const bf16* __restrict__ x, int64_t ldxb, int64_t ldxr, int B, int F, int L,
                   const uint4* __restrict__ wpack, const uint4* __restrict__ opack, bf16* __restrict__ y,
                   int64_t ldyb, int64_t ldyr, float* __restrict__ logit, int accumulate) {
  constexpr int NKC = (NMB + 1) / 2;  // 32-key chunks
  __shared__ __attribute__((aligned(16))) uint8_t lds[kAiMaxLayers * kAiLayerBytes + kAiOutBytes];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;

  {
    uint4* wl = reinterpret_cast<uint4*>(lds);
    for (int i = threadIdx.x; i < L * (kAiLayerBytes / 16); i += 64 * WAVES) wl[i] = wpack[i];
    if (opack) {
      uint4* ol = reinterpret_cast<uint4*>(lds + kAiMaxLayers * kAiLayerBytes);
      for (int i = threadIdx.x; i < NMB * 256; i += 64 * WAVES) ol[i] = opack[i];
    }
  }
  __syncthreads();

  const int step = gridDim.x * WAVES;
  int b = blockIdx.x * WAVES + wid;
  if (b >= B) return;

  // this lane's row of every block (clamped) and whether its keys exist
  int64_t roff[NMB];
  bool keyok[NMB][4];
#pragma unroll
  for (int mb = 0; mb < NMB; ++mb) {
    roff[mb] = int64_t(min(16 * mb + fr, F - 1)) * ldxr + 8 * fq;
#pragma unroll
    for (int i = 0; i < 4; ++i) keyok[mb][i] = 16 * mb + 4 * fq + i < F;
  }
  const bool half1 = (fq >> 1) != 0;  // 4 heads: this lane's units of a 32-chunk belong to the odd head

  bf16x8 xf[NMB][2], nx[NMB][2];
  auto load_x = [&](int bb, bf16x8(&r)[NMB][2]) {
    const bf16* base = x + int64_t(bb) * ldxb;
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) r[mb][kc] = *reinterpret_cast<const bf16x8*>(base + roff[mb] + 32 * kc);
  };
  load_x(b, xf);

  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (; b < B; b += step) {
    load_x(min(b + step, B - 1), nx);

    for (int l = 0; l < L; ++l) {
      // fragment (mat, ub, kc) of this layer: ((4 mat + ub) 2 + kc) 64 + lane
      const bf16x8* WF = reinterpret_cast<const bf16x8*>(lds + l * kAiLayerBytes) + lane;

      // Q^T and K^T, a pair of unit blocks at a time: the pair, rounded, is chunk g of the row
      bf16x8 qf[NMB][2], kf[NMB][2];
#pragma unroll
      for (int mat = 0; mat < 2; ++mat)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          __builtin_amdgcn_sched_barrier(0);  // keep later groups' fragment reads out of this one's registers
          f32x4 a[2][NMB];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const bf16x8 w0 = WF[((4 * mat + 2 * g + t) * 2) * 64], w1 = WF[((4 * mat + 2 * g + t) * 2 + 1) * 64];
#pragma unroll
            for (int mb = 0; mb < NMB; ++mb) a[t][mb] = ai_mfma(w1, xf[mb][1], ai_mfma(w0, xf[mb][0], zero4));
          }
#pragma unroll
          for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int i = 0; i < 4; ++i) (mat ? kf : qf)[mb][g][4 * t + i] = f2bf(a[t][mb][i]);
        }

      // V: unit position fr of block ub, keys 16 kb + 4 fq + i -> the A fragments of V^T
      bf16x8 vf[4][NKC];
#pragma unroll
      for (int ub = 0; ub < 4; ++ub) {
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8 w0 = WF[((8 + ub) * 2) * 64], w1 = WF[((8 + ub) * 2 + 1) * 64];
#pragma unroll
        for (int kb = 0; kb < 2 * NKC; ++kb) {
          f32x4 d = zero4;
          if (kb < NMB) d = ai_mfma(xf[kb][1], w1, ai_mfma(xf[kb][0], w0, zero4));
#pragma unroll
          for (int i = 0; i < 4; ++i) vf[ub][kb >> 1][4 * (kb & 1) + i] = f2bf(d[i]);
        }
      }

      // the O^T accumulators start from Wres^T x^T
      f32x4 acc[4][NMB];
#pragma unroll
      for (int ub = 0; ub < 4; ++ub) {
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8 w0 = WF[((12 + ub) * 2) * 64], w1 = WF[((12 + ub) * 2 + 1) * 64];
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) acc[ub][mb] = ai_mfma(w1, xf[mb][1], ai_mfma(w0, xf[mb][0], zero4));
      }

#pragma unroll
      for (int h = 0; h < HEADS; ++h) {
        const int g0 = HEADS == 1 ? 0 : (HEADS == 2 ? h : h >> 1);  // first 32-unit chunk of the head
        constexpr int NG = HEADS == 1 ? 2 : 1;                      // chunks of the head
        const bool mine = HEADS < 4 || half1 == bool(h & 1);         // 4 heads: the lane's units are this head's
#pragma unroll
        for (int qb = 0; qb < NMB; ++qb) {
          __builtin_amdgcn_sched_barrier(0);  // one (head, query block) at a time in the registers
          bf16x8 qh[NG];
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            qh[g] = qf[qb][g0 + g];
            if (HEADS == 4) {  // d = 16: zero the half of the 32-deep chunk that is the other head's
#pragma unroll
              for (int e = 0; e < 8; ++e) qh[g][e] = mine ? qh[g][e] : f2bf(0.f);
            }
          }
          f32x4 s[NMB];
          float mx = -INFINITY;
#pragma unroll
          for (int kb = 0; kb < NMB; ++kb) {
            s[kb] = zero4;
#pragma unroll
            for (int g = 0; g < NG; ++g) s[kb] = ai_mfma(kf[kb][g0 + g], qh[g], s[kb]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              s[kb][i] = keyok[kb][i] ? s[kb][i] : -INFINITY;
              mx = fmaxf(mx, s[kb][i]);
            }
          }
          mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
          mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // key 0 exists: finite
          float sum = 0.f;
          bf16x8 pf[NKC];
#pragma unroll
          for (int kb = 0; kb < 2 * NKC; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float e = 0.f;
              if (kb < NMB) {
                e = __expf(s[kb][i] - mx);
                sum += e;
              }
              pf[kb >> 1][4 * (kb & 1) + i] = f2bf(e);
            }
          sum += __shfl_xor(sum, 16, 64);
          sum += __shfl_xor(sum, 32, 64);
          const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
          for (int ub = 0; ub < 4; ++ub) {
            if (HEADS != 1 && (ub >> 1) != g0) continue;
            f32x4 o = zero4;
#pragma unroll
            for (int c = 0; c < NKC; ++c) o = ai_mfma(vf[ub][c], pf[c], o);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[ub][qb][i] = mine ? __builtin_fmaf(o[i], inv, acc[ub][qb][i]) : acc[ub][qb][i];
          }
        }
      }

      // relu, bf16: the next layer's x fragments
#pragma unroll
      for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) xf[mb][g][4 * t + i] = f2bf(fmaxf(acc[2 * g + t][mb][i], 0.f));
    }

    if (y) {
      bf16* yb = y + int64_t(b) * ldyb + 8 * fq;
#pragma unroll
      for (int mb = 0; mb < NMB; ++mb)
        if (16 * mb + fr < F) {
#pragma unroll
          for (int g = 0; g < 2; ++g)
            *reinterpret_cast<bf16x8*>(yb + int64_t(16 * mb + fr) * ldyr + 32 * g) = xf[mb][g];
        }
    }
    if (opack) {
      const f32x4* OF = reinterpret_cast<const f32x4*>(lds + kAiMaxLayers * kAiLayerBytes) + 2 * lane;
      float p = 0.f;
#pragma unroll
      for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const f32x4 w0 = OF[(2 * mb + g) * 128], w1 = OF[(2 * mb + g) * 128 + 1];
#pragma unroll
          for (int e = 0; e < 4; ++e) p = __builtin_fmaf(w0[e], bf2f(xf[mb][g][e]), p);
#pragma unroll
          for (int e = 0; e < 4; ++e) p = __builtin_fmaf(w1[e], bf2f(xf[mb][g][4 + e]), p);
        }
      p = wave_sum(p);
      if (lane == 0) logit[b] = accumulate ? logit[b] + p : p;
    }

#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) xf[mb][kc] = nx[mb][kc];
  }
}

}  // namespace kern

using namespace kern;

hipError_t launch_autoint(const void* x, int64_t ldxb, int64_t ldxr, int B, int F, int heads, int L, const void* wpack,
                          const float* opack, void* y, int64_t ldyb, int64_t ldyr, float* logit, bool accumulate,
                          hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (B < 0 || F < 1 || F > 64 || L < 1 || L > kAiMaxLayers || (heads != 1 && heads != 2 && heads != 4))
    return hipErrorInvalidValue;
  if (!x || !wpack || (opack != nullptr) != (logit != nullptr) || (!y && !logit)) return hipErrorInvalidValue;
  if (ldxb % 8 || ldxr % 8 || ldxr < 64 || reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(wpack) % 16 ||
      reinterpret_cast<uintptr_t>(opack) % 16)
    return hipErrorInvalidValue;
  if (y && (ldyb % 8 || ldyr % 8 || ldyr < 64 || reinterpret_cast<uintptr_t>(y) % 16)) return hipErrorInvalidValue;
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
      n = 256;
    cus = n;
  }
#define DTFS_AI(N, H, W)                                                                                          \
  hipLaunchKernelGGL((autoint_kernel<N, H, W>), dim3(std::min((B + W - 1) / W, cus)), dim3(64 * W), 0, st,          \
                     static_cast<const bf16*>(x), ldxb, ldxr, B, F, L, static_cast<const uint4*>(wpack),            \
                     reinterpret_cast<const uint4*>(opack), static_cast<bf16*>(y), ldyb, ldyr, logit, int(accumulate))
#define DTFS_AI_HEADS(N, W4) \
  if (heads == 1)            \
    DTFS_AI(N, 1, 8);        \
  else if (heads == 2)       \
    DTFS_AI(N, 2, 8);        \
  else                       \
    DTFS_AI(N, 4, W4)
  switch ((F + 15) / 16) {
    case 1: DTFS_AI_HEADS(1, 8); break;
    case 2: DTFS_AI_HEADS(2, 8); break;
    case 3: DTFS_AI_HEADS(3, 8); break;
    default: DTFS_AI_HEADS(4, 4); break;  // 4 blocks x 4 heads: one wave per SIMD (registers)
  }
#undef DTFS_AI_HEADS
#undef DTFS_AI
  return hipGetLastError();
}

}  // namespace dtfs
