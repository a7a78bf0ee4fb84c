// e4m3 code rows of the fp8 embedding tables -> bf16 operands, shared by the
// local-table kernels (interaction_fp8.hip) and the peer-lookup kernels
// (peer_lookup_fp8.hip).
#pragma once
#include "common.h"

namespace dtfs {
namespace kern {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// 8 e4m3 codes -> 8 bf16 values code * sc. v_cvt_pk_f32_fp8 (two codes per
// instruction, exact), an fp32 multiply by the power-of-two scale (exact) and
// the round to bf16 (exact: 4 significand bits fit bf16's 8). gfx950's
// v_cvt_scalef32_pk_bf16_fp8 would fold the three into one instruction; the
// kernels here wait on random 64-byte row reads, not on these ~16 VALU
// instructions per k-step, so the form whose rounding is plain C++ is kept.
__device__ __forceinline__ bf16x8 fp8x8_to_bf16(uint2 q, float sc) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(int(q.x), false);
  const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8(int(q.x), true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8(int(q.y), false);
  const f32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8(int(q.y), true);
  bf16x8 x;
  x[0] = f2bf(a[0] * sc);
  x[1] = f2bf(a[1] * sc);
  x[2] = f2bf(b[0] * sc);
  x[3] = f2bf(b[1] * sc);
  x[4] = f2bf(c[0] * sc);
  x[5] = f2bf(c[1] * sc);
  x[6] = f2bf(d[0] * sc);
  x[7] = f2bf(d[1] * sc);
  return x;
}

}  // namespace kern
}  // namespace dtfs
