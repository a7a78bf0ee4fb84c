// The fused MLP tail (mlp_tail.hip) on the block-scaled fp8 matrix cores:
//
//   (xq, sx)  = MX-fp8(x)                                   x bf16 [M, 1024]
//   h2        = act2((xq 2^sx) W2q^T * sw2 + b2)            fp32, never rounded to bf16
//   (h2q, s2) = MX-fp8(h2)
//   h3        = act3((h2q 2^s2) W3q^T * sw3 + b3)           fp32, registers
//   y[m]      = out_act(h3[m, :] . hw + hbias + sum_e extra[e][m])
//
// MX-fp8 = OCP e4m3 values + one E8M0 scale byte per (row, 32 consecutive
// columns): e = smallest integer with amax / 2^e <= 448 (0 for a zero block,
// clamped to [-127, 127]), q = e4m3(x 2^-e), byte = e + 127 - the rule of
// store_cross_mx (gemm.hip) and ops.quant_mx_fp8, bit for bit.
//
// One 512-thread workgroup owns 64 rows, as in mlp_tail.hip, and quantises
// its own operands: no quant_rows launch, no global round trip of xq or h2.
//
//   * the 64 x 1024 bf16 rows are read once (16 bytes per lane; a 32-column
//     block is 4 consecutive lanes, so its amax is two cross-lane maxes) and
//     written to LDS as e4m3 (64 KiB) + scale bytes (2 KiB), in 4 pieces of
//     256 columns: piece q + 1 is loaded to registers before the MFMAs of
//     piece q and quantised behind them (one barrier per piece).
//   * GEMM2: wave w owns h2 columns [64 w, 64 w + 64). A fragments come from
//     LDS, W2 fragments straight from global memory in fragment order
//     (ops.pack_bfrag_fp8), one 128-deep K tile ahead.
//   * GEMM2 epilogue: h2 = act2(acc * sw2 + b2); a lane holds 2 x 4 columns of
//     the 32-column block (tile pair j, j + 1), the 4 lanes of a row reduce
//     the block amax (xor-shuffle 16 / 32); e4m3 (32 KiB) + scales (1 KiB) to LDS.
//   * GEMM3 (wave w: h3 columns [32 w, 32 w + 32)) and the head as in mlp_tail.hip.
//
// MFMA: v_mfma_scale_f32_16x16x128_f8f6f4, transposed form (D = W_frag x
// A_frag^T: lane (fr, fq) holds C[m = fr][n = 4 fq .. + 3]). Operand layout
// (tools/native/mx_probe.hip): lane (fr, fq) holds row fr, K [16 fq, + 16) in
// its first 4 VGPRs and K [64 + 16 fq, + 16) in the last 4 - 16-byte chunks fq
// and fq + 4 of the 128-byte K tile - while the scale byte the lane supplies
// scales row fr's K block [32 fq, + 32): NOT the K range of its own data.
// The activations are the scaled operand; the weights carry the unit block
// scale 127 and their per-channel fp32 scale is applied in the epilogue.
//
// LDS images: 16-byte chunk c of row r sits at chunk c ^ (r & 15) of the row
// (row pitches are multiples of 256 bytes; the 16 rows of a ds_read_b128 lane
// group then land on 16 distinct 16-byte slots). Scale bytes are kept in the
// order they are consumed: [K tile][lane = 16 fq + fr][row tile i], so a lane
// reads the 4 scale bytes it feeds to the MFMAs of one K tile as one dword.
#include "common.h"
#include "launchers.h"

namespace dtfs {
namespace kern {

namespace {
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

// E8M0 exponent of a block: smallest e with amax / 2^e <= 448 (gemm.hip store_cross_mx)
__device__ __forceinline__ int mx_exponent(float amax) {
  int e = 0;
  if (amax > 0.f) {
    int ex;
    (void)frexpf(amax / 448.f, &ex);  // amax/448 = f * 2^ex, f in [0.5, 1)
    e = ex;
    if (ldexpf(448.f, e - 1) >= amax) e -= 1;
    e = max(-127, min(127, e));
  }
  return e;
}

__device__ __forceinline__ int pack_fp8x4(float a, float b, float c, float d) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return w;
}

// 16-byte chunks fq and fq + 4 of K tile kt of an e4m3 LDS image row
template <int PITCH>
__device__ __forceinline__ i32x8 mx_frag_lds(const uint8_t* img, int row, int kt, int fq) {
  const uint8_t* r = img + row * PITCH;
  const i32x4 lo = *reinterpret_cast<const i32x4*>(r + (((8 * kt + fq) ^ (row & 15)) << 4));
  const i32x4 hi = *reinterpret_cast<const i32x4*>(r + (((8 * kt + 4 + fq) ^ (row & 15)) << 4));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// weights: unit block scale; activations: the lane's real E8M0 byte
__device__ __forceinline__ f32x4 mx_mfma_act(const i32x8& w, const i32x8& a, const f32x4& c, int scale_a) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, a, c, 0, 0, 0, 127, 0, scale_a);
}
}  // namespace

template <int K1, int N2, int N3>
__global__ void __launch_bounds__(512) mlp_tail_fp8_kernel(const bf16* __restrict__ X, int64_t ldx, int M,
                                                           const i32x4* __restrict__ W2p, const float* __restrict__ sw2,
                                                           const float* __restrict__ b2, int act2,
                                                           const i32x4* __restrict__ W3p, const float* __restrict__ sw3,
                                                           const float* __restrict__ b3, int act3,
                                                           const float* __restrict__ hw, float hbias,
                                                           const float* __restrict__ extra, int extra_n,
                                                           int64_t extra_ld, int out_act, float* __restrict__ y) {
  constexpr int BM = 64, NW = 8;
  constexpr int NK1 = K1 / 128, NK2 = N2 / 128;  // K tiles of GEMM2 / GEMM3
  constexpr int TJ2 = N2 / NW / 16, TJ3 = N3 / NW / 16;
  constexpr int NQ = NK1 / 2;              // x is quantised in pieces of 2 K tiles (256 columns)
  constexpr int CPQ = 256 / 8;             // 16-byte bf16 chunks per row of a piece
  constexpr int RPI = 512 / CPQ;           // rows per pass of the 512 threads
  constexpr int XIT = BM / RPI;            // chunks per thread and piece
  static_assert(K1 % 256 == 0 && N2 % 128 == 0 && TJ2 % 2 == 0 && TJ2 * 16 * NW == N2 && TJ3 * 16 * NW == N3,
                "tail shape");
  static_assert(512 % CPQ == 0 && BM % RPI == 0, "piece split");
  __shared__ __attribute__((aligned(16))) uint8_t smem[BM * K1 + BM * (K1 / 32) + BM * N2 + BM * (N2 / 32) + NW * BM * 4];
  uint8_t* xq = smem;                          // [64][K1] e4m3, chunk-swizzled
  uint8_t* sxs = xq + BM * K1;                 // [kt][lane][i] scale bytes of xq
  uint8_t* h2q = sxs + BM * (K1 / 32);         // [64][N2] e4m3, chunk-swizzled
  uint8_t* s2s = h2q + BM * N2;                // [t][lane][i] scale bytes of h2q
  float* red = reinterpret_cast<float*>(s2s + BM * (N2 / 32));

  const int m0 = blockIdx.x * BM;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;

  // W2 fragments of this wave's columns: packed block (n16 = wid TJ2 + j, kt)
  // is 2 x 64 lanes x 16 bytes (half h: K chunk fq + 4 h)
  const i32x4* w2w = W2p + int64_t(wid * TJ2) * NK1 * 128 + lane;
  auto load_b2 = [&](i32x8(&b)[TJ2], int kt) {
#pragma unroll
    for (int j = 0; j < TJ2; ++j) {
      const i32x4 lo = w2w[(j * NK1 + kt) * 128];
      const i32x4 hi = w2w[(j * NK1 + kt) * 128 + 64];
      b[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
  };
  i32x8 bb0[TJ2], bb1[TJ2];

  // x -> MX-fp8 in LDS, a piece of 256 columns (2 K tiles) at a time: chunk
  // (row = 16 it + thread / 32, 8 columns at 256 q + 8 (thread % 32)); lanes
  // 4 k .. 4 k + 3 share a 32-column block. Rows past M read row M - 1 (their
  // scores are never stored). Piece q + 1 is in flight (registers) during
  // the MFMAs of piece q and is quantised behind them.
  const int cq = threadIdx.x % CPQ;
  const int r0 = threadIdx.x / CPQ;
  const bf16* xsrc[XIT];
#pragma unroll
  for (int it = 0; it < XIT; ++it) xsrc[it] = X + int64_t(min(m0 + it * RPI + r0, M - 1)) * ldx + cq * 8;
  bf16x8 xr[XIT];
  auto load_x = [&](int q) {
#pragma unroll
    for (int it = 0; it < XIT; ++it) xr[it] = *reinterpret_cast<const bf16x8*>(xsrc[it] + q * 256);
  };
  auto quant_x = [&](int q) {
    const int cc = q * CPQ + cq;  // 8-column chunk of the row
#pragma unroll
    for (int it = 0; it < XIT; ++it) {
      const int row = it * RPI + r0;
      float v[8];
      float amax = 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        v[u] = bf2f(xr[it][u]);
        amax = fmaxf(amax, fabsf(v[u]));
      }
      amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
      amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
      const int e = mx_exponent(amax);
      const float inv = ldexpf(1.f, -e);
      i32x2 qv;
      qv[0] = pack_fp8x4(v[0] * inv, v[1] * inv, v[2] * inv, v[3] * inv);
      qv[1] = pack_fp8x4(v[4] * inv, v[5] * inv, v[6] * inv, v[7] * inv);
      *reinterpret_cast<i32x2*>(xq + row * K1 + ((((cc >> 1) ^ (row & 15))) << 4) + (cc & 1) * 8) = qv;
      if ((cc & 3) == 0) {
        const int blk = cc >> 2;  // K tile blk >> 2, scale lane group blk & 3
        sxs[((blk >> 2) * 64 + (blk & 3) * 16 + (row & 15)) * 4 + (row >> 4)] = uint8_t(e + 127);
      }
    }
  };
  load_x(0);
  load_b2(bb0, 0);
  quant_x(0);
  if (NQ > 1) load_x(1);
  __syncthreads();

  // GEMM2: h2 = xq W2q^T over K1
  f32x4 acc[4][TJ2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < TJ2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto gemm2_tile = [&](int kt, const i32x8(&bc)[TJ2], i32x8(&bn)[TJ2]) {
    // the K loop is fully unrolled (static registers, exact waits): nothing
    // else orders the tiles, and without this fence the scheduler hoists
    // every tile's fragment reads to the top and spills
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < NK1) load_b2(bn, kt + 1);
    const uint32_t sw4 = *reinterpret_cast<const uint32_t*>(sxs + (kt * 64 + lane) * 4);
    i32x8 fa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = mx_frag_lds<K1>(xq, 16 * i + fr, kt, fq);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int sc = int((sw4 >> (8 * i)) & 0xffu);
#pragma unroll
      for (int j = 0; j < TJ2; ++j) acc[i][j] = mx_mfma_act(bc[j], fa[i], acc[i][j], sc);
    }
    // ... and sinks the MFMAs below the later pieces' barriers, keeping every
    // fragment live: pin the tile's results here
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < TJ2; ++j) asm volatile("" : "+v"(acc[i][j])::"memory");
  };
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    gemm2_tile(2 * q, bb0, bb1);
    gemm2_tile(2 * q + 1, bb1, bb0);
    if (q + 1 < NQ) {
      __builtin_amdgcn_sched_barrier(0);
      quant_x(q + 1);
      if (q + 2 < NQ) load_x(q + 2);
      __syncthreads();  // piece q + 1 is in LDS (each piece has its own region: no reuse hazard)
    }
  }

  // W3 fragments of this wave's columns, all of K2, in flight during the
  // GEMM2 epilogue (the W2 buffers are dead)
  const i32x4* w3w = W3p + int64_t(wid * TJ3) * NK2 * 128 + lane;
  i32x8 w3[NK2][TJ3];
#pragma unroll
  for (int t = 0; t < NK2; ++t)
#pragma unroll
    for (int j = 0; j < TJ3; ++j) {
      const i32x4 lo = w3w[(j * NK2 + t) * 128];
      const i32x4 hi = w3w[(j * NK2 + t) * 128 + 64];
      w3[t][j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }

  // GEMM2 epilogue: h2 = act2(acc * sw2 + b2) in fp32 -> MX-fp8 -> LDS.
  // Tile pair (j, j + 1) = the 32-column block n32 = 64 wid + 16 j.
  {
    const float lo = act2 == 1 ? 0.f : -__builtin_huge_valf();
#pragma unroll
    for (int j = 0; j < TJ2; j += 2) {
      f32x4 s4[2], b4[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int n = wid * (N2 / NW) + 16 * (j + h) + 4 * fq;
        s4[h] = *reinterpret_cast<const f32x4*>(sw2 + n);
        b4[h] = *reinterpret_cast<const f32x4*>(b2 + n);
      }
      const int blk = (wid * (N2 / NW) + 16 * j) / 32;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 16 * i + fr;
        float v[2][4];
        float amax = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            v[h][r] = fmaxf(acc[i][j + h][r] * s4[h][r] + b4[h][r], lo);
            amax = fmaxf(amax, fabsf(v[h][r]));
          }
        amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
        const int e = mx_exponent(amax);
        const float inv = ldexpf(1.f, -e);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int n = wid * (N2 / NW) + 16 * (j + h) + 4 * fq;
          *reinterpret_cast<int*>(h2q + m * N2 + (((n >> 4) ^ (m & 15)) << 4) + (n & 15)) =
              pack_fp8x4(v[h][0] * inv, v[h][1] * inv, v[h][2] * inv, v[h][3] * inv);
        }
        if (fq == 0) s2s[((blk >> 2) * 64 + (blk & 3) * 16 + fr) * 4 + i] = uint8_t(e + 127);
      }
    }
  }
  __syncthreads();

  // GEMM3: h3 = h2q W3q^T over K2 = N2
  f32x4 acc3[4][TJ3];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < TJ3; ++j) acc3[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < NK2; ++t) {
    const uint32_t sw4 = *reinterpret_cast<const uint32_t*>(s2s + (t * 64 + lane) * 4);
    i32x8 fa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = mx_frag_lds<N2>(h2q, 16 * i + fr, t, fq);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int sc = int((sw4 >> (8 * i)) & 0xffu);
#pragma unroll
      for (int j = 0; j < TJ3; ++j) acc3[i][j] = mx_mfma_act(w3[t][j], fa[i], acc3[i][j], sc);
    }
  }

  // head: per-row partial dot over this wave's N3 / 8 columns, then the 4
  // lanes of a row (xor 16, 32), then the 8 waves through LDS
  float part[4] = {0.f, 0.f, 0.f, 0.f};
  {
    const float lo = act3 == 1 ? 0.f : -__builtin_huge_valf();
#pragma unroll
    for (int j = 0; j < TJ3; ++j) {
      const int n = wid * (N3 / NW) + 16 * j + 4 * fq;
      const f32x4 s4 = *reinterpret_cast<const f32x4*>(sw3 + n);
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(b3 + n);
      const f32x4 h4 = *reinterpret_cast<const f32x4*>(hw + n);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[i] += fmaxf(acc3[i][j][r] * s4[r] + b4[r], lo) * h4[r];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v = part[i];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (fq == 0) red[wid * BM + 16 * i + fr] = v;
  }
  __syncthreads();
  if (threadIdx.x < BM) {
    const int row = threadIdx.x;
    const int m = m0 + row;
    if (m < M) {
      float s = hbias;
      for (int e = 0; extra && e < extra_n; ++e) s += extra[e * extra_ld + m];
#pragma unroll
      for (int w = 0; w < NW; ++w) s += red[w * BM + row];
      y[m] = out_act == 2 ? sigmoidf(s) : s;
    }
  }
}

}  // namespace kern

hipError_t launch_mlp_tail_fp8(const void* X, int64_t ldx, int M, int K1, const void* W2p, const float* sw2,
                               const float* b2, int act2, int N2, const void* W3p, const float* sw3, const float* b3,
                               int act3, int N3, const float* hw, float hbias, const float* extra, int extra_n,
                               int64_t extra_ld, int out_act, float* y, hipStream_t st) {
  if (M == 0) return hipSuccess;
  if (M < 0 || K1 != 1024 || N2 != 512 || N3 != 256 || ldx < K1 || (ldx & 7) || extra_n < 0 ||
      (extra && extra_n > 1 && extra_ld < M) || (act2 != 0 && act2 != 1) || (act3 != 0 && act3 != 1))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((kern::mlp_tail_fp8_kernel<1024, 512, 256>), dim3((M + 63) / 64), dim3(512), 0, st,
                     static_cast<const kern::bf16*>(X), ldx, M, static_cast<const kern::i32x4*>(W2p), sw2, b2, act2,
                     static_cast<const kern::i32x4*>(W3p), sw3, b3, act3, hw, hbias, extra, extra_n, extra_ld,
                     out_act, y);
  return hipGetLastError();
}

}  // namespace dtfs
