// DCN-v2 mixture of low-rank cross experts ("DCN-Mix"), one launch per layer:
//
//   a      = tanh(V xl)                    [M, R]   R = E r, bf16 in LDS
//   p      = softmax_i(G xl)               [M, E]   fp32
//   c_i    = tanh(C_i a_i)                 [M, r]   per expert slice
//   h      = concat_i(p_i c_i)             [M, R]   bf16 in LDS
//   z      = bf16(x0 * (U h + b) + xl)     [M, d]
//   logit  = sum_j float(z_j) head_w_j     [M]      (optional)
//
// sum_i p_i = 1 and b is shared, so sum_i p_i x0 * (U_i c_i + b) + xl is the
// one GEMM U h above: the [M, R] intermediates never leave the CU.
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
//
// One 512-thread workgroup owns 64 rows (the mlp_tail.hip pattern).
//
// Stage 1, [64, d] x [d, R_pad + gate]: xl's rows go through a 4-slot LDS
// ring of 64-deep K tiles (LDS-DMA, two tiles ahead, one barrier per tile);
// V is kept in pack_bfrag order and loaded per wave straight into registers
// one tile ahead. The R_pad / 16 column blocks are dealt as TJ columns x TI
// row blocks per wave: 8 column groups x all 4 row blocks when R_pad / 16 is
// a multiple of 8, else 4 column groups x 2 row groups (R_pad = 64, 192; V is
// then read by two waves, but no wave idles). The gate is one more 16-row
// block (G zero padded): its 2 x 4 (K half, row block) MFMAs of every K tile
// are dealt one to each wave, so the gate costs every wave one fragment load,
// one LDS read and one MFMA per tile; the two K halves meet in LDS. Every
// global load of the loop is inline asm (asm_io.h) and every vmcnt is placed
// by hand: d is a runtime value, and with compiler-tracked loads in a runtime
// loop the waitcnt pass drains the prefetch at the back edge.
//
// Stage 1b: softmax over E by one lane per row. The E r x r products read the
// `a` panel as the MFMA A operand and C as one block-diagonal [R_pad, R_pad]
// matrix in pack_bfrag order; only the 32-deep K chunks that overlap the
// expert's slice are visited (the rest of their columns are zero). tanh,
// times p_i, bf16, into the second panel.
//
// Stage 2, [64, R_pad] x [R_pad, d]: each wave keeps the whole h panel as
// fragments in registers (4 x R_pad / 32 of them) and takes 32-column pairs
// of 16-column blocks round-robin. U's rows are permuted on the host inside
// every 32-row group (block t, fragment row 4 q + s = U row 8 q + 4 t + s), so
// the MFMA's C layout leaves lane (fr, fq) with 8 consecutive columns of its
// row: x0, xl and z move 16 bytes per lane, 64 contiguous bytes per row per
// instruction, instead of the 8-byte pieces of the plain layout. The head dot
// is reduced across lanes and waves as in the tail kernel.
//
// Rows past M read row M - 1 and write nothing. Padded columns of V, C and U
// are zero, so a and h are exactly 0 there.
//
// MFMA: v_mfma_f32_16x16x32_bf16, D = W_frag x A_frag^T: lane (fr, fq) holds
// C[m = fr][n = 4 fq .. + 3].
#include "asm_io.h"
#include "common.h"
#include "launchers.h"

namespace dtfs {
namespace kern {

namespace {
// ring tile: 64 rows x 128 bytes, 16-byte chunk c of row r at c ^ ((r >> 1) & 7)
__device__ __forceinline__ int ring_swz(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// orders every later use of an asm-loaded fragment after the wait in front of it
__device__ __forceinline__ void landed(bf16x8& v) { asm volatile("" : "+v"(v)); }
}  // namespace

template <int NJ>  // R_pad = 64 NJ
__global__ void __launch_bounds__(512)
    cross_mix_kernel(const bf16* __restrict__ x0, int64_t ld0, const bf16* __restrict__ xl, int64_t ldl, int M, int d,
                     int E, int r, const bf16x8* __restrict__ Vp, const bf16x8* __restrict__ Gp,
                     const bf16x8* __restrict__ Cp, const bf16x8* __restrict__ Up, const float* __restrict__ bias,
                     const float* __restrict__ hw, bf16* __restrict__ z, int64_t ldz, float* __restrict__ logit) {
  constexpr int BM = 64, NW = 8, NS = 4, LEAD = 2, SLOT = BM * 128;
  constexpr int RP = 64 * NJ, PP = RP * 2;           // panel width (columns), row pitch (bytes)
  constexpr int SW = NJ % 2 == 0 ? 15 : 7;           // panel chunk swizzle: PP / 16 is a multiple of SW + 1
  constexpr int CW = NJ % 2 == 0 ? 8 : 4;            // stage 1 column groups
  constexpr int TJ = RP / 16 / CW, TI = 4 / (NW / CW);  // 16-column / 16-row blocks per wave
  constexpr int NC = 2 * NJ;                         // 32-deep K chunks of a panel
  __shared__ __attribute__((aligned(16))) uint8_t smem[NS * SLOT + 2 * BM * PP];
  __shared__ __attribute__((aligned(16))) float gpart[2][BM][16];  // gate logits of the two K halves
  __shared__ float ps[BM][8];                                      // softmax
  __shared__ float red[NW][BM];
  uint8_t* ring = smem;
  uint8_t* pa = smem + NS * SLOT;  // a panel
  uint8_t* ph = pa + BM * PP;      // h panel

  const int m0 = blockIdx.x * BM;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int nkt = d / 64;
  const int cg = wid % CW, rg = wid / CW;  // this wave's column group / row group
  const int gk = cg & 1, gi = rg * TI + (cg >> 1);  // its share of the gate block: K half, row block
  auto panel = [&](uint8_t* p, int m, int chunk) { return p + m * PP + ((chunk ^ (m & SW)) << 4); };

  // ---------------------------------------------------------------- stage 1
  const int ar = 8 * wid + (lane >> 3);
  const bf16* a_src = xl + int64_t(min(m0 + ar, M - 1)) * ldl + (((lane & 7) ^ ((ar >> 1) & 7)) << 3);
  const uint32_t ring_lds = lds_addr(ring) + wid * 1024;
  auto stage_a = [&](int kt) { lds_dma16(a_src + min(kt, nkt - 1) * 64, ring_lds + (kt % NS) * SLOT); };
  const bf16x8* vw = Vp + int64_t(cg * TJ) * nkt * 128 + lane;
  const bf16x8* gw = Gp + gk * 64 + lane;
  auto load_b = [&](bf16x8(&b)[TJ][2], bf16x8& g, int kt) {
    const int kc = min(kt, nkt - 1);  // trailing loads repeat the last tile (branch-free loop)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) b[j][kk] = gload16(vw + ((j * nkt + kc) * 2 + kk) * 64);
    g = gload16(gw + kc * 128);
  };

  f32x4 acc[TI][TJ], gacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // K tile kt: issue B(kt + 1), G(kt + 1), A(kt + 2); the queue then ends
  // ... B(kt) G(kt) | A(kt + 1) B(kt + 1) G(kt + 1) A(kt + 2), so vmcnt(2 TJ + 3)
  // leaves only the part right of the bar in flight (A(kt) is older still).
  // WAR on the ring as in mlp_tail.hip: slot (kt + 2) % 4 was last read in
  // iteration kt - 2, which every wave left before the barrier of kt - 1.
  auto body = [&](int kt, bf16x8(&bc)[TJ][2], bf16x8& gc, bf16x8(&bn)[TJ][2], bf16x8& gn) {
    load_b(bn, gn, kt + 1);
    stage_a(kt + LEAD);
    wait_vm<2 * TJ + 3>();
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      landed(bc[j][0]);
      landed(bc[j][1]);
    }
    landed(gc);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (kt < nkt) {  // odd nkt: the pair's second half only keeps the pipeline's counts
      const uint8_t* as = ring + (kt % NS) * SLOT;
      bf16x8 fa[2][TI];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < TI; ++i)
          fa[kk][i] = *reinterpret_cast<const bf16x8*>(as + ring_swz(16 * (rg * TI + i) + fr, 4 * kk + fq));
      const bf16x8 fg = *reinterpret_cast<const bf16x8*>(as + ring_swz(16 * gi + fr, 4 * gk + fq));
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bc[j][kk], fa[kk][i], acc[i][j], 0, 0, 0);
      gacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gc, fg, gacc, 0, 0, 0);
    }
  };
  {
    bf16x8 bb0[TJ][2], bb1[TJ][2], g0, g1;
    stage_a(0);
    load_b(bb0, g0, 0);
    stage_a(1);
    for (int kt = 0; kt < nkt; kt += 2) {
      body(kt, bb0, g0, bb1, g1);
      body(kt + 1, bb1, g1, bb0, g0);
    }
    wait_vm<0>();  // the trailing loads and ring stages land before anything else
    landed(g0);
    landed(g1);
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        landed(bb0[j][kk]);
        landed(bb1[j][kk]);
      }
  }

  // a = bf16(tanh(acc)) -> panel; gate partial logits -> LDS
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int n = 16 * (cg * TJ + j) + 4 * fq;
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const int m = 16 * (rg * TI + i) + fr;
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf(tanhf(acc[i][j][e]));
      *reinterpret_cast<bf16x4*>(panel(pa, m, n >> 3) + (n & 7) * 2) = o;
    }
  }
  *reinterpret_cast<f32x4*>(&gpart[gk][16 * gi + fr][4 * fq]) = gacc;
  __syncthreads();

  // --------------------------------------------------------------- stage 1b
  if (threadIdx.x < BM) {
    const int row = threadIdx.x;
    float l[8], mx = -__builtin_huge_valf(), s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      l[e] = e < E ? gpart[0][row][e] + gpart[1][row][e] : -__builtin_huge_valf();
      mx = fmaxf(mx, l[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      l[e] = e < E ? expf(l[e] - mx) : 0.f;
      s += l[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) ps[row][e] = l[e] / s;
  }
  const int R = E * r;
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int jb = cg * TJ + j;
#pragma unroll
    for (int i = 0; i < TI; ++i) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (16 * jb >= R) continue;  // padding columns: h = 0
    const int k0 = (16 * jb) / r * r;  // the expert's slice [k0, k0 + r)
    for (int kc = k0 / 32; kc < (k0 + r + 31) / 32; ++kc) {
      const bf16x8 cf = Cp[(jb * NC + kc) * 64 + lane];
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(panel(pa, 16 * (rg * TI + i) + fr, 4 * kc + fq));
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cf, af, acc[i][j], 0, 0, 0);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int n = 16 * (cg * TJ + j) + 4 * fq;
    const int e = min(n / r, E - 1);
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const int m = 16 * (rg * TI + i) + fr;
      const float p = ps[m][e];
      bf16x4 o;
#pragma unroll
      for (int t = 0; t < 4; ++t) o[t] = f2bf(tanhf(acc[i][j][t]) * p);
      *reinterpret_cast<bf16x4*>(panel(ph, m, n >> 3) + (n & 7) * 2) = o;
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- stage 2
  bf16x8 hf[4][NC];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int kc = 0; kc < NC; ++kc) hf[i][kc] = *reinterpret_cast<const bf16x8*>(panel(ph, 16 * i + fr, 4 * kc + fq));

  int64_t o0[4], ol[4], oz[4];  // this lane's row offsets (elements); rows past M read row M - 1
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = min(m0 + 16 * i + fr, M - 1);
    o0[i] = m * ld0;
    ol[i] = m * ldl;
    oz[i] = m * ldz;
  }
  float part[4] = {0.f, 0.f, 0.f, 0.f};
  for (int pr = wid; pr < d / 32; pr += NW) {
    f32x4 y[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bf16x8* uw = Up + int64_t(2 * pr + t) * NC * 64 + lane;
      bf16x8 uf[NC];
#pragma unroll
      for (int kc = 0; kc < NC; ++kc) uf[kc] = uw[kc * 64];
#pragma unroll
      for (int i = 0; i < 4; ++i) y[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < NC; ++kc)
#pragma unroll
        for (int i = 0; i < 4; ++i) y[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(uf[kc], hf[i][kc], y[t][i], 0, 0, 0);
    }
    const int c0 = 32 * pr + 8 * fq;  // this lane's 8 columns: y[0][i] then y[1][i]
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bias + c0), b1 = *reinterpret_cast<const f32x4*>(bias + c0 + 4);
    f32x4 h0 = {0.f, 0.f, 0.f, 0.f}, h1 = h0;
    if (hw) {
      h0 = *reinterpret_cast<const f32x4*>(hw + c0);
      h1 = *reinterpret_cast<const f32x4*>(hw + c0 + 4);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bf16x8 v0 = *reinterpret_cast<const bf16x8*>(x0 + o0[i] + c0);
      const bf16x8 vl = *reinterpret_cast<const bf16x8*>(xl + ol[i] + c0);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = f2bf(bf2f(v0[e]) * (y[0][i][e] + b0[e]) + bf2f(vl[e]));
        o[4 + e] = f2bf(bf2f(v0[4 + e]) * (y[1][i][e] + b1[e]) + bf2f(vl[4 + e]));
        part[i] += bf2f(o[e]) * h0[e] + bf2f(o[4 + e]) * h1[e];
      }
      if (z && m0 + 16 * i + fr < M) *reinterpret_cast<bf16x8*>(z + oz[i] + c0) = o;
    }
  }
  if (!logit) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v = part[i];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (fq == 0) red[wid][16 * i + fr] = v;
  }
  __syncthreads();
  if (threadIdx.x < BM && m0 + int(threadIdx.x) < M) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w][threadIdx.x];
    logit[m0 + threadIdx.x] = s;
  }
}

}  // namespace kern

hipError_t launch_cross_mix(const void* x0, int64_t ld0, const void* xl, int64_t ldl, int M, int d, int E, int r,
                            const void* Vp, const void* Gp, const void* Cp, const void* Up, const float* bias,
                            const float* hw, void* z, int64_t ldz, float* logit, hipStream_t st) {
  if (M == 0) return hipSuccess;
  if (M < 0 || d < 64 || d % 64 || r < 16 || r % 16 || E < 1 || E > 8 || E * r > 256 || (!z && !logit) ||
      (logit && !hw))
    return hipErrorInvalidValue;
  const int NJ = (E * r + 63) / 64;
#define DTFS_CROSS_MIX(N)                                                                                          \
  hipLaunchKernelGGL((kern::cross_mix_kernel<N>), dim3((M + 63) / 64), dim3(512), 0, st,                           \
                     static_cast<const kern::bf16*>(x0), ld0, static_cast<const kern::bf16*>(xl), ldl, M, d, E, r, \
                     static_cast<const kern::bf16x8*>(Vp), static_cast<const kern::bf16x8*>(Gp),                   \
                     static_cast<const kern::bf16x8*>(Cp), static_cast<const kern::bf16x8*>(Up), bias, hw,         \
                     static_cast<kern::bf16*>(z), ldz, logit)
  switch (NJ) {
    case 1: DTFS_CROSS_MIX(1); break;
    case 2: DTFS_CROSS_MIX(2); break;
    case 3: DTFS_CROSS_MIX(3); break;
    default: DTFS_CROSS_MIX(4); break;
  }
#undef DTFS_CROSS_MIX
  return hipGetLastError();
}

}  // namespace dtfs
