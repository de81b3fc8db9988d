// Element-wise pieces of a Llama-style decoder layer for gfx950: rotary position embedding of Q and
// K, and the SwiGLU activation of the MLP.  Both are memory-bound: every tensor is read once and
// written once in 16-byte vectors, the math is fp32 with ONE rounding to bf16.
//
// rope_qk: out = x * cos + rotate_half(x) * sin for q [B,H,T,D] and k [B,Hkv,T,D] in one launch
//   (any batch / head / token strides: transposed views of [B,T,H*D] projections, slices of a
//   packed projection), written to [B,T,H,D] / [B,T,Hkv,D] memory.  cos / sin are [Bc,T,D] (Bc in
//   {1, B}), fp32 or bf16, and ARBITRARY: the two halves of a row are not assumed equal.  With
//   h = D / 2:   out[i]     = x[i]     * cos[i]     - x[i + h] * sin[i]
//                out[i + h] = x[i + h] * cos[i + h] + x[i]     * sin[i + h]
//   and the backward (same kernel, template flag) is the transposed map
//                dx[i]      = g[i]     * cos[i]     + g[i + h] * sin[i + h]
//                dx[i + h]  = g[i + h] * cos[i + h] - g[i]     * sin[i].
//   Work split: one wave owns one token (b, t), a 256-thread block four tokens.  A lane owns one
//   8-element chunk of the first half of a head row AND the matching chunk of the second half (two
//   16-byte loads), so the rotation partner is always in the same lane: no LDS, no cross-lane
//   traffic.  D / 16 lanes cover a head, a wave 16 (D = 64) or 8 (D = 128) heads per pass; the
//   passes run over the H query heads and then the Hkv key heads as one head index (the last pass
//   is ragged, the Q -> K switch may fall inside a pass).  The lane's cos / sin chunks are loaded
//   once, held as fp32 in 32 registers and reused by every pass: cos / sin traffic is 1 / (H + Hkv)
//   of the tensor traffic.
//
// swiglu: y = gate * sigmoid(gate) * up over [M, I] bf16 rows (a row stride each: the halves of a
//   packed [M, 2I] gate-up projection are valid inputs), grid-stride over 8-element vectors.  The
//   backward reads dy, gate, up once and writes dgate and dup:
//     s = 1 / (1 + exp(-g)),  dup = dy * g * s,  dgate = dy * u * s * (1 + g * (1 - s))
//   (exp overflow for g << 0 gives s = 1 / inf = 0, never NaN).

#include "common.h"

namespace damd {
namespace dec {

__device__ __forceinline__ void ld8(const bf16_t* p, float (&f)[8]) {
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = bf2f(v.v[j]);
}

__device__ __forceinline__ void ld8(const float* p, float (&f)[8]) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

__device__ __forceinline__ void st8(bf16_t* p, const float (&f)[8]) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    const u16v2_t r = f2bf2(f[j], f[j + 1]);
    o.v[j] = r[0];
    o.v[j + 1] = r[1];
  }
  *reinterpret_cast<bf16x8*>(p) = o;
}

struct RopeArgs {
  const bf16_t* q;  // [B,H,T,D] view: element strides qb, qh, qt (D contiguous)
  const bf16_t* k;  // [B,Hkv,T,D] view
  bf16_t* oq;       // [B,T,H,D] contiguous
  bf16_t* ok;       // [B,T,Hkv,D] contiguous
  const void* cos;  // [Bc,T,D]: element strides cb (0 when Bc == 1), ct
  const void* sin;
  int64_t qb, qh, qt, kb, kh, kt, cb, ct, sb, st;
  int64_t tokens;  // B * T
  int T, H, Hkv;
};

constexpr int kRopeThreads = 256;
constexpr int kRopeTokens = kRopeThreads / kWave;  // tokens per block

template <int D, bool BWD, typename CS>
__global__ void __launch_bounds__(kRopeThreads) rope_qk_kernel(const RopeArgs a) {
  constexpr int kHalf = D / 2;
  constexpr int kLanesPerHead = D / 16;
  constexpr int kHeadsPerPass = kWave / kLanesPerHead;
  const int64_t tok = static_cast<int64_t>(blockIdx.x) * kRopeTokens + (threadIdx.x >> 6);
  if (tok >= a.tokens) return;  // whole waves leave; nothing below synchronises
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t b = tok / a.T, t = tok % a.T;
  const int i0 = (lane % kLanesPerHead) * 8;  // this lane's chunk of the first half; partner at i0 + kHalf

  float c1[8], c2[8], s1[8], s2[8];
  {
    const CS* c = static_cast<const CS*>(a.cos) + b * a.cb + t * a.ct + i0;
    const CS* s = static_cast<const CS*>(a.sin) + b * a.sb + t * a.st + i0;
    ld8(c, c1);
    ld8(c + kHalf, c2);
    ld8(s, s1);
    ld8(s + kHalf, s2);
  }

  const bf16_t* qrow = a.q + b * a.qb + t * a.qt + i0;
  const bf16_t* krow = a.k + b * a.kb + t * a.kt + i0;
  bf16_t* oqrow = a.oq + tok * a.H * D + i0;
  bf16_t* okrow = a.ok + tok * a.Hkv * D + i0;
  const int heads = a.H + a.Hkv;
  for (int hh = lane / kLanesPerHead; hh < heads; hh += kHeadsPerPass) {
    const bool isq = hh < a.H;
    const int h = isq ? hh : hh - a.H;
    const bf16_t* src = isq ? qrow + h * a.qh : krow + h * a.kh;
    bf16_t* dst = (isq ? oqrow : okrow) + static_cast<int64_t>(h) * D;
    float x1[8], x2[8], o1[8], o2[8];
    ld8(src, x1);
    ld8(src + kHalf, x2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (BWD) {
        o1[j] = x1[j] * c1[j] + x2[j] * s2[j];
        o2[j] = x2[j] * c2[j] - x1[j] * s1[j];
      } else {
        o1[j] = x1[j] * c1[j] - x2[j] * s1[j];
        o2[j] = x2[j] * c2[j] + x1[j] * s2[j];
      }
    }
    st8(dst, o1);
    st8(dst + kHalf, o2);
  }
}

__device__ __forceinline__ float sigmoidf(float g) { return 1.f / (1.f + __expf(-g)); }

// Vector i of the [M, I / 8] grid sits at row i / vpr, column vector i % vpr; the row / column pair
// is advanced incrementally (one 64-bit division per thread, none in the loop).
struct RowCol {
  int64_t row;
  int col;
  int drow, dcol;  // the grid stride as (rows, column vectors)
  int vpr;
  __device__ __forceinline__ RowCol(int64_t i, int64_t stride, int vpr_) : vpr(vpr_) {
    row = i / vpr;
    col = static_cast<int>(i % vpr);
    drow = static_cast<int>(stride / vpr);
    dcol = static_cast<int>(stride % vpr);
  }
  __device__ __forceinline__ void next() {
    row += drow;
    col += dcol;
    if (col >= vpr) {
      col -= vpr;
      ++row;
    }
  }
};

__global__ void __launch_bounds__(256)
swiglu_fwd_kernel(const bf16_t* __restrict__ gate, const bf16_t* __restrict__ up, bf16_t* __restrict__ y, int64_t nvec,
                  int vpr, int64_t gs, int64_t us) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  for (RowCol rc(i, stride, vpr); i < nvec; i += stride, rc.next()) {
    float g[8], u[8], o[8];
    ld8(gate + rc.row * gs + rc.col * 8, g);
    ld8(up + rc.row * us + rc.col * 8, u);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = g[j] * sigmoidf(g[j]) * u[j];
    st8(y + i * 8, o);
  }
}

__global__ void __launch_bounds__(256)
swiglu_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ gate, const bf16_t* __restrict__ up,
                  bf16_t* __restrict__ dgate, bf16_t* __restrict__ dup, int64_t nvec, int vpr, int64_t gs, int64_t us) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  for (RowCol rc(i, stride, vpr); i < nvec; i += stride, rc.next()) {
    float d[8], g[8], u[8], dg[8], du[8];
    ld8(dy + i * 8, d);
    ld8(gate + rc.row * gs + rc.col * 8, g);
    ld8(up + rc.row * us + rc.col * 8, u);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float s = sigmoidf(g[j]);
      du[j] = d[j] * g[j] * s;
      dg[j] = d[j] * u[j] * s * (1.f + g[j] * (1.f - s));
    }
    st8(dgate + i * 8, dg);
    st8(dup + i * 8, du);
  }
}

// One resident set of workgroups (8 x 256 threads per CU), grid-stride beyond that.
inline unsigned stream_grid(int64_t nvec) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    DAMD_CHECK(hipGetDevice(&dev));
    DAMD_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    cus = n > 0 ? n : 256;
  }
  const int64_t want = (nvec + 255) / 256, cap = int64_t{cus} * 8;
  return static_cast<unsigned>(want < cap ? want : cap);
}

template <int D, bool BWD>
void rope_launch_cs(const RopeArgs& a, int cs_bf16, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>((a.tokens + kRopeTokens - 1) / kRopeTokens));
  if (cs_bf16)
    DAMD_LAUNCH((rope_qk_kernel<D, BWD, bf16_t>), grid, dim3(kRopeThreads), 0, st, a);
  else
    DAMD_LAUNCH((rope_qk_kernel<D, BWD, float>), grid, dim3(kRopeThreads), 0, st, a);
}

}  // namespace dec
}  // namespace damd

using namespace damd;
using namespace damd::dec;

extern "C" {

// q / k: [B,H|Hkv,T,D] bf16 views, strides[0..2] = q (batch, head, token), [3..5] = k, [6..7] = cos
// (batch -- 0 for a shared table --, token), [8..9] = sin; oq / ok: contiguous [B,T,H|Hkv,D].
void damd_rope_qk_launch(const void* q, const void* k, void* oq, void* ok, const void* cos, const void* sin,
                         const int64_t* strides, int B, int T, int H, int Hkv, int D, int cs_bf16, int backward,
                         hipStream_t st) {
  if (B <= 0 || T <= 0 || H + Hkv <= 0) return;
  RopeArgs a;
  a.q = static_cast<const bf16_t*>(q);
  a.k = static_cast<const bf16_t*>(k);
  a.oq = static_cast<bf16_t*>(oq);
  a.ok = static_cast<bf16_t*>(ok);
  a.cos = cos;
  a.sin = sin;
  a.qb = strides[0]; a.qh = strides[1]; a.qt = strides[2];
  a.kb = strides[3]; a.kh = strides[4]; a.kt = strides[5];
  a.cb = strides[6]; a.ct = strides[7];
  a.sb = strides[8]; a.st = strides[9];
  a.tokens = static_cast<int64_t>(B) * T;
  a.T = T;
  a.H = H;
  a.Hkv = Hkv;
  if (D == 64) {
    if (backward) rope_launch_cs<64, true>(a, cs_bf16, st);
    else rope_launch_cs<64, false>(a, cs_bf16, st);
  } else {  // D == 128 (checked by the binding)
    if (backward) rope_launch_cs<128, true>(a, cs_bf16, st);
    else rope_launch_cs<128, false>(a, cs_bf16, st);
  }
}

// gate / up: [M, I] bf16 with row strides gs / us (elements), I % 8 == 0; y: contiguous [M, I]
void damd_swiglu_fwd_launch(const void* gate, const void* up, void* y, int64_t M, int I, int64_t gs, int64_t us,
                            hipStream_t st) {
  const int vpr = I / 8;
  const int64_t nvec = M * vpr;
  if (nvec <= 0) return;
  DAMD_LAUNCH(swiglu_fwd_kernel, dim3(stream_grid(nvec)), dim3(256), 0, st, static_cast<const bf16_t*>(gate),
              static_cast<const bf16_t*>(up), static_cast<bf16_t*>(y), nvec, vpr, gs, us);
}

// dy, dgate, dup: contiguous [M, I]
void damd_swiglu_bwd_launch(const void* dy, const void* gate, const void* up, void* dgate, void* dup, int64_t M, int I,
                            int64_t gs, int64_t us, hipStream_t st) {
  const int vpr = I / 8;
  const int64_t nvec = M * vpr;
  if (nvec <= 0) return;
  DAMD_LAUNCH(swiglu_bwd_kernel, dim3(stream_grid(nvec)), dim3(256), 0, st, static_cast<const bf16_t*>(dy),
              static_cast<const bf16_t*>(gate), static_cast<const bf16_t*>(up), static_cast<bf16_t*>(dgate),
              static_cast<bf16_t*>(dup), nvec, vpr, gs, us);
}

}  // extern "C"
