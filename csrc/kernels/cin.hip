// xDeepFM Compressed Interaction Network (Lian et al. 2018), one layer per launch:
//
//   X^k[b,h,d] = bf16(bias[h] + sum_{i < H_prev} sum_{j < F} W[h,i,j] * Z[b,i,j,d])
//   Z[b,i,j,d] = bf16(X^{k-1}[b,i,d] * X^0[b,j,d])
//   logit[b]  (+)= sum_h w_out[h] * sum_d float(X^k[b,h,d])
//
// As a GEMM: M = (b, d), K = (i, j), N = h. The activation operand Z is the
// outer product of two small per-candidate tiles and exists only in
// registers: K is ordered on the host so that one 32-deep K step is 4 values
// of i (step t: i = 4 t + fq) times one 8-wide block of j (j = 8 jb + s), and
// the MFMA's lane (fr, fq), which supplies 8 consecutive k of its row, forms
// its fragment as one scalar X^{k-1}[b, 4 t + fq, d] times the 8-vector
// X^0[b, 8 jb .. + 7, d]: 8 fp32 multiplies (a product of two bf16 values is
// exact in fp32) and one round-to-nearest-even conversion. The fragment feeds
// all H / 16 column blocks.
//
// One 512-thread workgroup owns 8 candidates, one per wave. A wave's 64 d's
// are four 16-row blocks; MFMA row fr of block rb is d = 4 fr + rb, so
//   * the lane's four scalars of a step are 8 contiguous bytes of X^{k-1}
//     (one global_load_dwordx2; the wave reads four whole 128-byte maps), and
//   * the C layout leaves the lane with d = 4 fr .. 4 fr + 3 of output map h:
//     the 16 lanes of a quad write the full 128-byte row of (b, h).
// X^0[b] is kept d-major ([d][j], 128-byte rows, 16-byte chunk jb stored at
// jb ^ (fr & 7)) in LDS, 8 KB per wave: the 8-vector is one ds_read_b128.
//
// W streams through a 4-slot LDS ring of one K step each (NCP fragments of
// 1 KB in pack_bfrag order: lane (fr, fq) holds W[16 nc + fr, 4 t + fq,
// 8 jb .. + 7]), LDS-DMA two steps ahead, one barrier per step, every vmcnt
// placed by hand (the cross_mix.hip stage-1 pattern; trailing steps repeat the
// last tile so the loop is branch-free). Wave w stages fragment w % NCP: below
// 8 column blocks some fragments are staged twice (same bytes, same address),
// which keeps every wave's vmcnt the same. Each step also issues the wave's
// X^{k-1} load of the next step (L1 hits while t stays).
//
// Accumulators: 4 row blocks x NCP column blocks x 4 fp32, 128 registers at
// NCP = 8, for the whole K loop. H > 128 runs ceil(H / 128) column passes of
// NCP = ceil(H / 16 / passes) blocks; Z is regenerated per pass.
//
// Traffic: every workgroup reads all of W, 2 K H bytes for 8 candidates'
// 2 * 8 * 64 * K * H FLOP: 1 / 512 byte per FLOP out of L2 (1.5 MB of W for
// layer 2 of the preset, L2 resident), i.e. 2 TB/s at 1 PFLOP/s.
//
// Padding: i >= H_prev contributes an exact 0 (the scalar is zeroed; its load
// is clamped into the row), j >= F is 0 in the LDS tile, padded W is 0, maps
// H <= h < H_pad are written as exact zeros. Candidates past B read candidate
// B - 1 and write nothing. logit[b] has one writer, lane 0 of b's wave.
//
// MFMA: v_mfma_f32_16x16x32_bf16, D = W_frag x Z_frag^T: lane (fr, fq) holds
// C[m = fr][n = 4 fq .. + 3].
#include "asm_io.h"
#include "common.h"
#include "launchers.h"

namespace dtfs {
namespace kern {

namespace {
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// 8 bytes per lane global -> registers; volatile: keeps its place among the LDS-DMAs
__device__ __forceinline__ bf16x4 gload8(const void* g) {
  bf16x4 v;
  asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(v) : "v"(g));
  return v;
}
// orders every later use of an asm-loaded value after the wait in front of it
__device__ __forceinline__ void landed(bf16x4& v) { asm volatile("" : "+v"(v)); }
}  // namespace

template <int NCP>  // 16-column blocks per pass
__global__ void __launch_bounds__(512)
    cin_kernel(const bf16* __restrict__ x0, int64_t ld0, const bf16* __restrict__ xp, int64_t ldp, int B, int F,
               int HP, int H, int npass, const bf16x8* __restrict__ Wp, const float* __restrict__ bias,
               const float* __restrict__ wout, bf16* __restrict__ xk, int64_t ldk, float* __restrict__ logit,
               int accumulate) {
  constexpr int NW = 8, NS = 4, LEAD = 2, SLOT = NCP * 1024;
  __shared__ __attribute__((aligned(16))) uint8_t ring[NS * SLOT];
  __shared__ __attribute__((aligned(16))) uint8_t xt[NW][64 * 128];  // X^0 of the wave's candidate, [d][j]

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int64_t b = int64_t(blockIdx.x) * NW + wid;
  const bool live = b < B;
  const int64_t bc = live ? b : int64_t(B) - 1;
  const int JB = (F + 7) / 8, IT = (HP + 3) / 4, NK = IT * JB;
  const int HPAD = (H + 15) / 16 * 16;

  // X^0 tile: lane d gathers its 8 j of every block (128 contiguous bytes per j across the wave)
  uint8_t* my = xt[wid];
  {
    const bf16* src = x0 + bc * ld0 + lane;
    for (int jb = 0; jb < JB; ++jb) {
      bf16x8 v;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const bf16 t = src[min(8 * jb + s, F - 1) * 64];  // clamped, then selected: never past the row
        v[s] = 8 * jb + s < F ? t : f2bf(0.f);
      }
      *reinterpret_cast<bf16x8*>(my + lane * 128 + ((jb ^ ((lane >> 2) & 7)) << 4)) = v;
    }
  }
  __syncthreads();

  const bf16* xrow = xp + bc * ldp + 4 * fr;
  const int wf = wid % NCP;
  const uint32_t ring_lds = lds_addr(ring) + wf * 1024;
  float part = 0.f;

  for (int ps = 0; ps < npass; ++ps) {
    const bf16x8* wsrc = Wp + (int64_t(ps) * NK * NCP + wf) * 64 + lane;
    auto stage_w = [&](int ks) { lds_dma16(wsrc + int64_t(min(ks, NK - 1)) * NCP * 64, ring_lds + (ks % NS) * SLOT); };
    auto load_x = [&](int t) { return gload8(xrow + min(4 * min(t, IT - 1) + fq, HP - 1) * 64); };

    f32x4 acc[4][NCP];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int nc = 0; nc < NCP; ++nc) acc[rb][nc] = f32x4{0.f, 0.f, 0.f, 0.f};

    int tc = 0, jc = 0;  // (t, jb) of the current step
    // Step ks: issue X(ks + 1), W(ks + 2); the queue then ends
    // ... W(ks) X(ks) | W(ks + 1) X(ks + 1) W(ks + 2), so vmcnt(3) leaves only
    // the part right of the bar in flight. WAR on the ring: slot (ks + 2) % 4
    // was last read in step ks - 2, which every wave left before the barrier
    // of step ks - 1.
    auto body = [&](int ks, bf16x4& xc, bf16x4& xn) {
      int tn = tc, jn = jc + 1;
      if (jn == JB) {
        jn = 0;
        ++tn;
      }
      xn = load_x(tn);
      stage_w(ks + LEAD);
      wait_vm<3>();
      landed(xc);
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (ks < NK) {  // odd NK: the pair's second half only keeps the pipeline's counts
        const bool iv = 4 * tc + fq < HP;
        bf16x8 fa[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
          const float xs = iv ? bf2f(xc[rb]) : 0.f;
          const bf16x8 v = *reinterpret_cast<const bf16x8*>(my + (4 * fr + rb) * 128 + ((jc ^ (fr & 7)) << 4));
#pragma unroll
          for (int s = 0; s < 8; ++s) fa[rb][s] = f2bf(bf2f(v[s]) * xs);
        }
        const uint8_t* ws = ring + (ks % NS) * SLOT + lane * 16;
#pragma unroll
        for (int nc = 0; nc < NCP; ++nc) {
          const bf16x8 wfr = *reinterpret_cast<const bf16x8*>(ws + nc * 1024);
#pragma unroll
          for (int rb = 0; rb < 4; ++rb)
            acc[rb][nc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr, fa[rb], acc[rb][nc], 0, 0, 0);
        }
      }
      tc = tn;
      jc = jn;
    };
    {
      bf16x4 xa, xb;
      stage_w(0);
      xa = load_x(0);
      stage_w(1);
      for (int ks = 0; ks < NK; ks += 2) {
        body(ks, xa, xb);
        body(ks + 1, xb, xa);
      }
      wait_vm<0>();  // the trailing loads and ring stages land before anything else
      landed(xa);
      landed(xb);
    }

    // bias, bf16, the map's row of (b, h); p[b, h] over this lane's 4 d's
#pragma unroll
    for (int nc = 0; nc < NCP; ++nc)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int h = 16 * (ps * NCP + nc) + 4 * fq + e;
        const bool hv = h < H;
        const int hc = min(h, H - 1);  // clamped, then selected: no branch per column
        const float bl = bias[hc], wl = wout[hc];
        const float bv = hv ? bl : 0.f, wv = hv ? wl : 0.f;
        bf16x4 o;
        float s = 0.f;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
          o[rb] = f2bf(acc[rb][nc][e] + bv);
          s += bf2f(o[rb]);
        }
        part += wv * s;
        if (xk && live && h < HPAD) *reinterpret_cast<bf16x4*>(xk + b * ldk + h * 64 + 4 * fr) = o;
      }
    wait_vm<0>();
    __syncthreads();  // the next pass restarts the ring
  }

  part = wave_sum(part);
  if (lane == 0 && live) logit[b] = accumulate ? logit[b] + part : part;
}

}  // namespace kern

hipError_t launch_cin_layer(const void* x0, int64_t ld0, const void* xp, int64_t ldp, int B, int F, int H_prev, int H,
                            const void* Wp, const float* bias, const float* w_out, void* xk, int64_t ldk,
                            float* logit, bool accumulate, hipStream_t st) {
  if (B == 0) return hipSuccess;
  if (B < 0 || F < 1 || F > 64 || H_prev < 1 || H_prev > 256 || H < 1 || H > 256 || !logit) return hipErrorInvalidValue;
  const int npass = cin_passes(H);
#define DTFS_CIN(N)                                                                                             \
  hipLaunchKernelGGL((kern::cin_kernel<N>), dim3((B + 7) / 8), dim3(512), 0, st,                                \
                     static_cast<const kern::bf16*>(x0), ld0, static_cast<const kern::bf16*>(xp), ldp, B, F,    \
                     H_prev, H, npass, static_cast<const kern::bf16x8*>(Wp), bias, w_out,                       \
                     static_cast<kern::bf16*>(xk), ldk, logit, accumulate ? 1 : 0)
  switch (cin_pass_blocks(H)) {
    case 1: DTFS_CIN(1); break;
    case 2: DTFS_CIN(2); break;
    case 3: DTFS_CIN(3); break;
    case 4: DTFS_CIN(4); break;
    case 5: DTFS_CIN(5); break;
    case 6: DTFS_CIN(6); break;
    case 7: DTFS_CIN(7); break;
    default: DTFS_CIN(8); break;
  }
#undef DTFS_CIN
  return hipGetLastError();
}

}  // namespace dtfs
