// Element-wise pieces of a Llama-style decoder layer for gfx950: rotary position embedding of Q and
// K (alone, or fused with Qwen3's per-head Q / K RMSNorm), and the SwiGLU activation of the MLP.  All
// are memory-bound: every tensor is read once and
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
// rope_norm: the same map applied to the per-head RMS-normalised rows (Qwen3's q_norm / k_norm, an
//   RMSNorm over D of every query and key head before the rotation), still one read and one write:
//                r = rsqrt(mean_j(x_j^2) + eps),  y_i = w_i * x_i * r,  out = rope(y)
//   with [D] weights wq / wk (bf16 or fp32).  Limits as rope_qk: D in {64, 128}, bf16 q / k with any
//   batch / head / token strides, cos / sin fp32 or bf16 [Bc,T,D].  It keeps rope_qk's work split, which
//   makes the row reduction cheap: the D / 16 lanes of a head are an aligned group of 4 or 8 lanes, so
//   sum(x^2) is 16 local squares and 2 or 3 DPP butterfly steps (head_sum), no LDS.  The pass loop has a
//   wave-uniform trip count -- a lane past the last head carries zeros and stores nothing -- so every
//   lane takes part in the cross-lane steps.  cos / sin and BOTH weights are held as fp32 registers
//   (a lane sees query and key heads; the Q -> K switch selects per lane).
//   Backward, g the gradient of out, r recomputed from x (nothing saved for it):
//                gy = rope^T(g),  c = mean_j(w_j * gy_j * x_j),  dx_i = r * w_i * gy_i - x_i * r^3 * c
//                dw_i = sum over all (batch, token, head) rows of gy_i * x_i * r       (q and k separately)
//   The two row sums share the butterfly.  dw is deterministic, no atomics: a lane's chunk position is
//   fixed (lane % (D / 16)), so it accumulates its 16 dwq and 16 dwk values in registers over the passes
//   AND over tokens -- the grid is persistent (the workgroups resident at once, each wave grid-striding
//   over the tokens), which amortises the final reduction: the lanes of a wave that own the same chunk
//   (xor shuffles), the block's four waves (LDS, one barrier -- every wave reaches it, none returns
//   early), one fp32 [2, D] partial per workgroup, summed in a fixed order and rounded to the weight
//   dtype by norm.hip's wgrad_finalize kernels (as a [blocks, 2 * D] column sum).
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

struct RopeNormArgs {
  RopeArgs r;        // q, k: the projection outputs x; oq, ok: out (forward) or dq, dk (backward)
  const bf16_t* gq;  // backward only: the upstream gradients, [B,H,T,D] / [B,Hkv,T,D] views like q / k
  const bf16_t* gk;
  int64_t gqb, gqh, gqt, gkb, gkh, gkt;
  const void* wq;  // [D] norm weights, bf16 or fp32
  const void* wk;
  float* part;  // backward only: [gridDim.x, 2, D] weight-gradient partials
  float eps;
};

template <int CTRL>
__device__ __forceinline__ float dpp_add(float x) {
  return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}

// Sum over the aligned group of L (4 or 8) lanes that cover one head row, the same bits in every lane
// of the group: quad_perm xor 1, quad_perm xor 2 and, for 8 lanes, row_half_mirror (after the quad
// steps every lane of a quad holds the quad's sum, so lane 7 - i stands in for lane i ^ 4).
template <int L>
__device__ __forceinline__ float head_sum(float x) {
  x = dpp_add<0xB1>(x);
  x = dpp_add<0x4E>(x);
  if (L == 8) x = dpp_add<0x141>(x);
  return x;
}

template <int D, typename CS, typename WT>
__global__ void __launch_bounds__(kRopeThreads) rope_norm_fwd_kernel(const RopeNormArgs n) {
  constexpr int kHalf = D / 2;
  constexpr int kLanesPerHead = D / 16;
  constexpr int kHeadsPerPass = kWave / kLanesPerHead;
  const RopeArgs& a = n.r;
  const int64_t tok = static_cast<int64_t>(blockIdx.x) * kRopeTokens + (threadIdx.x >> 6);
  if (tok >= a.tokens) return;  // whole waves leave; nothing below synchronises across waves
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t b = tok / a.T, t = tok % a.T;
  const int i0 = (lane % kLanesPerHead) * 8;

  float c1[8], c2[8], s1[8], s2[8], wq1[8], wq2[8], wk1[8], wk2[8];
  {
    const CS* c = static_cast<const CS*>(a.cos) + b * a.cb + t * a.ct + i0;
    const CS* s = static_cast<const CS*>(a.sin) + b * a.sb + t * a.st + i0;
    ld8(c, c1);
    ld8(c + kHalf, c2);
    ld8(s, s1);
    ld8(s + kHalf, s2);
    ld8(static_cast<const WT*>(n.wq) + i0, wq1);
    ld8(static_cast<const WT*>(n.wq) + i0 + kHalf, wq2);
    ld8(static_cast<const WT*>(n.wk) + i0, wk1);
    ld8(static_cast<const WT*>(n.wk) + i0 + kHalf, wk2);
  }

  const bf16_t* qrow = a.q + b * a.qb + t * a.qt + i0;
  const bf16_t* krow = a.k + b * a.kb + t * a.kt + i0;
  bf16_t* oqrow = a.oq + tok * a.H * D + i0;
  bf16_t* okrow = a.ok + tok * a.Hkv * D + i0;
  const int heads = a.H + a.Hkv;
  // wave-uniform trip count: every lane takes part in the cross-lane steps, a lane past the last head
  // (its whole group is) carries zeros and stores nothing
  for (int h0 = 0; h0 < heads; h0 += kHeadsPerPass) {
    const int hh = h0 + lane / kLanesPerHead;
    const bool live = hh < heads, isq = hh < a.H;
    const int h = isq ? hh : hh - a.H;
    float x1[8] = {}, x2[8] = {}, o1[8], o2[8];
    if (live) {
      const bf16_t* src = isq ? qrow + h * a.qh : krow + h * a.kh;
      ld8(src, x1);
      ld8(src + kHalf, x2);
    }
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += x1[j] * x1[j] + x2[j] * x2[j];
    const float r = rsqrtf(head_sum<kLanesPerHead>(ss) * (1.f / D) + n.eps);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float y1 = (isq ? wq1[j] : wk1[j]) * x1[j] * r, y2 = (isq ? wq2[j] : wk2[j]) * x2[j] * r;
      o1[j] = y1 * c1[j] - y2 * s1[j];
      o2[j] = y2 * c2[j] + y1 * s2[j];
    }
    if (live) {
      bf16_t* dst = (isq ? oqrow : okrow) + static_cast<int64_t>(h) * D;
      st8(dst, o1);
      st8(dst + kHalf, o2);
    }
  }
}

template <int D, typename CS, typename WT>
__global__ void __launch_bounds__(kRopeThreads) rope_norm_bwd_kernel(const RopeNormArgs n) {
  constexpr int kHalf = D / 2;
  constexpr int kLanesPerHead = D / 16;
  constexpr int kHeadsPerPass = kWave / kLanesPerHead;
  static_assert(kRopeTokens == 4, "the block reduction below sums four waves");
  __shared__ float red[kRopeTokens][2][D];
  const RopeArgs& a = n.r;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int i0 = (lane % kLanesPerHead) * 8;

  float wq1[8], wq2[8], wk1[8], wk2[8];
  ld8(static_cast<const WT*>(n.wq) + i0, wq1);
  ld8(static_cast<const WT*>(n.wq) + i0 + kHalf, wq2);
  ld8(static_cast<const WT*>(n.wk) + i0, wk1);
  ld8(static_cast<const WT*>(n.wk) + i0 + kHalf, wk2);
  float dwq1[8] = {}, dwq2[8] = {}, dwk1[8] = {}, dwk2[8] = {};  // this lane's chunk of dw, summed over its tokens

  const int heads = a.H + a.Hkv;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kRopeTokens;
  // a wave with no token (left) skips the loop and still reaches the block reduction below
  for (int64_t tok = static_cast<int64_t>(blockIdx.x) * kRopeTokens + wave; tok < a.tokens; tok += step) {
    const int64_t b = tok / a.T, t = tok % a.T;
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
    const bf16_t* gqrow = n.gq + b * n.gqb + t * n.gqt + i0;
    const bf16_t* gkrow = n.gk + b * n.gkb + t * n.gkt + i0;
    bf16_t* dqrow = a.oq + tok * a.H * D + i0;
    bf16_t* dkrow = a.ok + tok * a.Hkv * D + i0;
    for (int h0 = 0; h0 < heads; h0 += kHeadsPerPass) {  // wave-uniform, as in the forward
      const int hh = h0 + lane / kLanesPerHead;
      const bool live = hh < heads, isq = hh < a.H;
      const int h = isq ? hh : hh - a.H;
      float x1[8] = {}, x2[8] = {}, g1[8] = {}, g2[8] = {};
      if (live) {
        const bf16_t* src = isq ? qrow + h * a.qh : krow + h * a.kh;
        const bf16_t* gsrc = isq ? gqrow + h * n.gqh : gkrow + h * n.gkh;
        ld8(src, x1);
        ld8(src + kHalf, x2);
        ld8(gsrc, g1);
        ld8(gsrc + kHalf, g2);
      }
      float w1[8], w2[8], ss = 0.f, cs = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float y1 = g1[j] * c1[j] + g2[j] * s2[j], y2 = g2[j] * c2[j] - g1[j] * s1[j];  // gy = rope^T(g)
        g1[j] = y1;
        g2[j] = y2;
        w1[j] = isq ? wq1[j] : wk1[j];
        w2[j] = isq ? wq2[j] : wk2[j];
        ss += x1[j] * x1[j] + x2[j] * x2[j];
        cs += w1[j] * y1 * x1[j] + w2[j] * y2 * x2[j];
      }
      const float r = rsqrtf(head_sum<kLanesPerHead>(ss) * (1.f / D) + n.eps);
      const float r3c = r * r * r * (head_sum<kLanesPerHead>(cs) * (1.f / D));
      float o1[8], o2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o1[j] = r * w1[j] * g1[j] - x1[j] * r3c;
        o2[j] = r * w2[j] * g2[j] - x2[j] * r3c;
        const float t1 = g1[j] * x1[j] * r, t2 = g2[j] * x2[j] * r;  // zero in a lane past the last head
        dwq1[j] += isq ? t1 : 0.f;
        dwq2[j] += isq ? t2 : 0.f;
        dwk1[j] += isq ? 0.f : t1;
        dwk2[j] += isq ? 0.f : t2;
      }
      if (live) {
        bf16_t* dst = (isq ? dqrow : dkrow) + static_cast<int64_t>(h) * D;
        st8(dst, o1);
        st8(dst + kHalf, o2);
      }
    }
  }

  // the lanes of a wave that own the same chunk (equal lane % kLanesPerHead), then the block's four
  // waves through LDS, always in the same order: the partial of a block is a function of its tokens
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int o = kLanesPerHead; o < kWave; o <<= 1) {
      dwq1[j] += __shfl_xor(dwq1[j], o, kWave);
      dwq2[j] += __shfl_xor(dwq2[j], o, kWave);
      dwk1[j] += __shfl_xor(dwk1[j], o, kWave);
      dwk2[j] += __shfl_xor(dwk2[j], o, kWave);
    }
  }
  if (lane < kLanesPerHead) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[wave][0][i0 + j] = dwq1[j];
      red[wave][0][i0 + kHalf + j] = dwq2[j];
      red[wave][1][i0 + j] = dwk1[j];
      red[wave][1][i0 + kHalf + j] = dwk2[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * D) {
    const float* p = &red[0][0][0] + threadIdx.x;
    n.part[static_cast<int64_t>(blockIdx.x) * 2 * D + threadIdx.x] = ((p[0] + p[2 * D]) + p[4 * D]) + p[6 * D];
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
inline int cu_count() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    DAMD_CHECK(hipGetDevice(&dev));
    DAMD_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    cus = n > 0 ? n : 256;
  }
  return cus;
}

inline unsigned stream_grid(int64_t nvec) {
  const int64_t want = (nvec + 255) / 256, cap = int64_t{cu_count()} * 8;
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

// Upper bound of the backward's grid (the rows of its workspace): a workgroup per four tokens up to 8 per CU.
inline unsigned rope_norm_bwd_grid_max(int64_t tokens) { return stream_grid(tokens * kWave); }

// Launches one instantiation and returns its grid.  The backward's grid is persistent: the workgroups
// that are resident at once (the instantiation's register use decides how many fit a CU), every wave
// grid-striding over the tokens.
template <int D, bool BWD, typename CS, typename WT>
unsigned rope_norm_launch_one(const RopeNormArgs& n, hipStream_t st) {
  unsigned grid = static_cast<unsigned>((n.r.tokens + kRopeTokens - 1) / kRopeTokens);
  if constexpr (BWD) {
    static int per_cu = 0;
    if (per_cu == 0) {
      int nb = 0;
      DAMD_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, rope_norm_bwd_kernel<D, CS, WT>, kRopeThreads, 0));
      per_cu = nb > 0 ? nb : 1;
    }
    const int64_t resident = int64_t{cu_count()} * per_cu, most = rope_norm_bwd_grid_max(n.r.tokens);
    grid = static_cast<unsigned>(resident < most ? resident : most);
    DAMD_LAUNCH((rope_norm_bwd_kernel<D, CS, WT>), dim3(grid), dim3(kRopeThreads), 0, st, n);
  } else {
    DAMD_LAUNCH((rope_norm_fwd_kernel<D, CS, WT>), dim3(grid), dim3(kRopeThreads), 0, st, n);
  }
  return grid;
}

template <int D, bool BWD>
unsigned rope_norm_launch(const RopeNormArgs& n, int cs_bf16, int w_bf16, hipStream_t st) {
  if (cs_bf16 && w_bf16) return rope_norm_launch_one<D, BWD, bf16_t, bf16_t>(n, st);
  if (cs_bf16) return rope_norm_launch_one<D, BWD, bf16_t, float>(n, st);
  if (w_bf16) return rope_norm_launch_one<D, BWD, float, bf16_t>(n, st);
  return rope_norm_launch_one<D, BWD, float, float>(n, st);
}

// strides[0..2] = q (batch, head, token), [3..5] = k, [6..7] = cos (batch -- 0 for a shared table --,
// token), [8..9] = sin
inline RopeArgs rope_args(const void* q, const void* k, void* oq, void* ok, const void* cos, const void* sin,
                          const int64_t* strides, int B, int T, int H, int Hkv) {
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
  return a;
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
  const RopeArgs a = rope_args(q, k, oq, ok, cos, sin, strides, B, T, H, Hkv);
  if (D == 64) {
    if (backward) rope_launch_cs<64, true>(a, cs_bf16, st);
    else rope_launch_cs<64, false>(a, cs_bf16, st);
  } else {  // D == 128 (checked by the binding)
    if (backward) rope_launch_cs<128, true>(a, cs_bf16, st);
    else rope_launch_cs<128, false>(a, cs_bf16, st);
  }
}

// rope(rms_norm(q, wq), rms_norm(k, wk)) with the norm over D: q / k / oq / ok / cos / sin / strides as
// in damd_rope_qk_launch; wq, wk: contiguous [D], bf16 (w_bf16) or fp32.  B, T > 0 (checked by the binding).
void damd_rope_norm_fwd_launch(const void* q, const void* k, void* oq, void* ok, const void* cos, const void* sin,
                               const void* wq, const void* wk, const int64_t* strides, int B, int T, int H, int Hkv,
                               int D, int cs_bf16, int w_bf16, float eps, hipStream_t st) {
  RopeNormArgs n = {};
  n.r = rope_args(q, k, oq, ok, cos, sin, strides, B, T, H, Hkv);
  n.wq = wq;
  n.wk = wk;
  n.eps = eps;
  if (D == 64) rope_norm_launch<64, false>(n, cs_bf16, w_bf16, st);
  else rope_norm_launch<128, false>(n, cs_bf16, w_bf16, st);
}

// Rows to allocate for the [rows, 2, D] fp32 workspace of damd_rope_norm_bwd_launch (one per workgroup at most).
int damd_rope_norm_bwd_blocks(int64_t tokens) { return static_cast<int>(rope_norm_bwd_grid_max(tokens)); }

// The backward of the above: gq / gk are the upstream gradients ([B,H|Hkv,T,D] views, strides[10..12] /
// [13..15] = batch, head, token), dq / dk contiguous [B,T,H|Hkv,D]; part receives each workgroup's
// [2, D] (dwq | dwk) partial.  Returns the number of partial rows written, for
// damd_norm_wgrad_finalize_launch to sum.
int damd_rope_norm_bwd_launch(const void* gq, const void* gk, const void* q, const void* k, void* dq, void* dk,
                               const void* cos, const void* sin, const void* wq, const void* wk, float* part,
                               const int64_t* strides, int B, int T, int H, int Hkv, int D, int cs_bf16, int w_bf16,
                               float eps, hipStream_t st) {
  RopeNormArgs n = {};
  n.r = rope_args(q, k, dq, dk, cos, sin, strides, B, T, H, Hkv);
  n.gq = static_cast<const bf16_t*>(gq);
  n.gk = static_cast<const bf16_t*>(gk);
  n.gqb = strides[10]; n.gqh = strides[11]; n.gqt = strides[12];
  n.gkb = strides[13]; n.gkh = strides[14]; n.gkt = strides[15];
  n.wq = wq;
  n.wk = wk;
  n.part = part;
  n.eps = eps;
  return static_cast<int>(D == 64 ? rope_norm_launch<64, true>(n, cs_bf16, w_bf16, st)
                                  : rope_norm_launch<128, true>(n, cs_bf16, w_bf16, st));
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
