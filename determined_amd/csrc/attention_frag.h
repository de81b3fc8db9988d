// MFMA fragment helpers shared by the attention kernels (attention.hip, attention_decode.hip,
// attention_chunk.hip): the vector types, the 16x16x32 bf16 MFMA, hardware bf16 conversion, the
// cross-row reductions of the S^T layout and the transposed LDS reads.  The fragment layout is described at the top of
// attention.hip.
#pragma once

#include "common.h"

namespace damd {
namespace attn {

typedef short s8 __attribute__((ext_vector_type(8)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s4 lds_s4;

constexpr int kBlk = 64;       // kv tile (fwd) / key block (bwd) / query block (bwd)
constexpr int kThreads = 256;  // 4 waves
constexpr float kLog2e = 1.4426950408889634f;
// LDS row stride of the staged K/V/Q/dO tiles: D + 16 elements makes both the row-major
// ds_read_b128 operand reads (lane groups {0-3,12-15,20-27}, ...) and the transposed
// ds_read_b64_tr_b16 reads (2 x 32 lanes) bank-conflict-free; D + 8 was 2-way on both
// (SQ_LDS_BANK_CONFLICT ~40% of LDS cycles).
constexpr int kLdsStride(int D) { return D + 16; }
constexpr float kLn2 = 0.6931471805599453f;

struct Strides {
  int64_t b, h, t;
};

__device__ __forceinline__ f4 mfma(s8 a, s8 b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
}

typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef short sh2 __attribute__((ext_vector_type(2)));

// gfx950 converts fp32 -> bf16 (round to nearest even) in hardware: one v_cvt_pk_bf16_f32 per
// pair instead of the ~6-instruction software rounding (the kernels are VALU-bound, not MFMA).
__device__ __forceinline__ sh2 cvt2(float a, float b) {
  return __builtin_bit_cast(sh2, __builtin_convertvector((f2{a, b}), bf2));
}
__device__ __forceinline__ short bfs(float x) { return cvt2(x, 0.f)[0]; }
// raw v_exp_f32 (softmax arguments are <= 0 or -inf; no denormal-range fixup needed)
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// Logit soft cap (y = c * tanh(z / c)): t = tanh(z / c) from x = z / c * 2 * log2(e) as 1 - 2 / (1 + 2^x),
// one v_exp_f32 + one v_rcp_f32; d = 1 - t^2 = 4r(1 - r) with r = 1 / (1 + 2^x), the backward's factor,
// without the cancellation of 1 - t*t.  2^x overflows to inf for large x: r = 0, t = 1, d = 0 -- no NaN.
__device__ __forceinline__ float cap_tanh(float x, float& d) {
  const float r = __builtin_amdgcn_rcpf(1.f + ex2(x));
  d = 4.f * r * (1.f - r);
  return fmaf(-2.f, r, 1.f);
}
// host side, cap c > 0 (0: none): the kernels' tanh argument is s * k1, their exp2 scale k2 = c * log2(e)
inline float cap_k1(float scale, float c) { return c > 0.f ? 2.f * kLog2e * scale / c : 0.f; }
__device__ __forceinline__ float cap_tanh(float x) { return fmaf(-2.f, __builtin_amdgcn_rcpf(1.f + ex2(x)), 1.f); }

// max / sum over the four 16-lane rows of a wave (lanes c, c+16, c+32, c+48): two VALU lane swaps
// (v_permlane16_swap, v_permlane32_swap) instead of two LDS round trips through ds_bpermute
__device__ __forceinline__ float rows_max(float x) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  const float y = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(y), __float_as_uint(y), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float rows_sum(float x) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  const float y = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(y), __float_as_uint(y), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

__device__ __forceinline__ s8 cat4(s4 lo, s4 hi) {
  s8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

// bf16 fragment from two 16-wide accumulator tiles (the permuted 32-wide k step).
__device__ __forceinline__ s8 pack_pair(f4 lo, f4 hi) {
  const sh2 a = cvt2(lo[0], lo[1]), b = cvt2(lo[2], lo[3]), c = cvt2(hi[0], hi[1]), d = cvt2(hi[2], hi[3]);
  s8 r;
  r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1];
  r[4] = c[0]; r[5] = c[1]; r[6] = d[0]; r[7] = d[1];
  return r;
}

__device__ __forceinline__ s4 tr_read(const bf16_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(p));
}

// Transposed operand (rows of the image are the k index): lane c of each 16-lane group gets
// column col0 + c of image rows {r0 + q} (elements 0..3) and {r1 + q} (elements 4..7).
__device__ __forceinline__ s8 tr_pair(const bf16_t* img, int stride, int r0, int r1, int col0, int c) {
  const int q = c >> 2, p = c & 3;
  const s4 lo = tr_read(img + (r0 + q) * stride + col0 + 4 * p);
  const s4 hi = tr_read(img + (r1 + q) * stride + col0 + 4 * p);
  return cat4(lo, hi);
}

}  // namespace attn
}  // namespace damd
