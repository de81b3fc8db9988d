// Fused language-model head loss and elementwise helpers for gfx950.
//
// lm_ce: next-token cross-entropy straight from the bf16 LM-head GEMM output
//   logits [B*T, Vp] (Vp = vocabulary padded for the GEMM, V = valid vocabulary),
//   labels [B*T] (int64; the label of row (b, t) is labels[b, t+1], the last position of
//   each sequence and label == ignore_index contribute nothing).
//   forward: one workgroup per row, ONE pass over the row with an online (max, sum) per
//            thread (16-byte loads), block merge -> row loss and log-sum-exp;
//   backward: dlogits = (softmax - onehot) * (dloss / n_valid), written as bf16, optionally
//            in place over the logits (they are dead after the loss), padded columns -> 0.
//   Replaces: slice + reshape + bf16->fp32 copy + softmax fwd + softmax bwd + fills.
//
// bias_grad: column sums of a [M, N] bf16 gradient (the bias gradient of a Linear) with
//   16-byte loads into row-split fp32 partials; the wide finalize of norm.hip finishes them.
//
// gelu (tanh approximation: GPT-2 MLP; exact erf form: BERT) after a Linear: forward g = gelu(h) as one vectorised
//   pass; backward dh = gelu'(h) * dg FUSED with the bias gradient of that Linear -- the
//   column partials of dh are accumulated while dh is written, so dh is never re-read for
//   the bias (replaces torch's GeluBackward + a separate column-sum pass).

#include "common.h"

#include <math.h>

namespace damd {
namespace fused {

constexpr int kCEThreads = 256;

__device__ __forceinline__ void online_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;
  s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
  m = mn;
}

__global__ void __launch_bounds__(kCEThreads)
lm_ce_fwd_kernel(const bf16_t* __restrict__ logits, const int64_t* __restrict__ labels, int T, int V, int Vp,
                 int64_t ignore_index, float* __restrict__ row_loss, float* __restrict__ lse_out) {
  const int64_t row = blockIdx.x;
  const int t = static_cast<int>(row % T);
  const bf16_t* x = logits + row * Vp;
  int64_t lab = t + 1 < T ? labels[row + 1] : ignore_index;
  if (lab == ignore_index || lab < 0 || lab >= V) lab = -1;
  float m = -INFINITY, s = 0.f;
  const int nvec = V / 8;
  for (int i = threadIdx.x; i < nvec; i += kCEThreads) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + i * 8);
    float f[8];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = bf2f(v.v[j]);
      mx = fmaxf(mx, f[j]);
    }
    // all eight masked (-inf): exp(-inf - -inf) would be NaN; exp(-inf - 0) = 0 adds nothing
    // (a select, not a `continue`: the branch cost ce_fwd_kernel 4%, profiles/ce_fwd_inf_guard_ab.txt)
    const float mz = mx == -INFINITY ? 0.f : mx;
    float ls = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ls += __expf(f[j] - mz);
    online_merge(m, s, mx, ls);
  }
  for (int i = nvec * 8 + threadIdx.x; i < V; i += kCEThreads) online_merge(m, s, bf2f(x[i]), 1.f);
  // wave merge
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    online_merge(m, s, m2, s2);
  }
  __shared__ float sm[kCEThreads / 64], ss[kCEThreads / 64];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sm[w] = m;
    ss[w] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0], S = ss[0];
    for (int k = 1; k < kCEThreads / 64; ++k) online_merge(M, S, sm[k], ss[k]);
    const float lse = M + logf(S);
    lse_out[row] = lse;
    row_loss[row] = lab >= 0 ? lse - bf2f(x[lab]) : 0.f;
  }
}

__global__ void __launch_bounds__(kCEThreads)
lm_ce_bwd_kernel(const bf16_t* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ lse,
                 const float* __restrict__ scale_ptr, int T, int V, int Vp, int64_t ignore_index,
                 bf16_t* __restrict__ dlogits) {
  const int64_t row = blockIdx.x;
  const int t = static_cast<int>(row % T);
  int64_t lab = t + 1 < T ? labels[row + 1] : ignore_index;
  const bool valid = !(lab == ignore_index || lab < 0 || lab >= V);
  const bf16_t* x = logits + row * Vp;
  bf16_t* dx = dlogits + row * Vp;
  const float scale = valid ? *scale_ptr : 0.f;
  const float L = lse[row];
  const int nvec = Vp / 8;
  for (int i = threadIdx.x; i < nvec; i += kCEThreads) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + i * 8);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = i * 8 + j;
      float g = 0.f;
      if (col < V && scale != 0.f) {
        g = __expf(bf2f(v.v[j]) - L);
        if (col == lab) g -= 1.f;
        g *= scale;
      }
      o.v[j] = f2bf(g);
    }
    *reinterpret_cast<bf16x8*>(dx + i * 8) = o;
  }
  for (int col = nvec * 8 + threadIdx.x; col < Vp; col += kCEThreads) {
    float g = 0.f;
    if (col < V && scale != 0.f) {
      g = __expf(bf2f(x[col]) - L);
      if (col == lab) g -= 1.f;
      g *= scale;
    }
    dx[col] = f2bf(g);
  }
}

// ---- token-classification cross-entropy (masked-LM heads): rows of V bf16 logits, one label per
// row (no shift), V even (rows are 4-byte aligned: bf16 pairs; BERT's V = 30522 is not a multiple
// of 8).  Rows whose label is ignore_index (85% of a masked-LM batch) are skipped by the forward
// and get a zero gradient row in the backward, so the forward reads only the labelled rows and
// nothing of the [rows, V] logits is ever converted to fp32.
typedef __bf16 bfv2 __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float2 ld_bf2(const bf16_t* p) {
  const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
  return make_float2(__uint_as_float(u << 16), __uint_as_float(u & 0xFFFF0000u));
}

__global__ void __launch_bounds__(kCEThreads)
ce_fwd_kernel(const bf16_t* __restrict__ logits, const int64_t* __restrict__ labels, int V, int64_t ignore_index,
              float* __restrict__ row_loss, float* __restrict__ lse_out) {
  const int64_t row = blockIdx.x;
  const int64_t lab = labels[row];
  if (lab == ignore_index || lab < 0 || lab >= V) {  // uniform per block
    if (threadIdx.x == 0) {
      row_loss[row] = 0.f;
      lse_out[row] = 0.f;
    }
    return;
  }
  const bf16_t* x = logits + row * V;
  float m = -INFINITY, s = 0.f;
  const int npair = V / 2;
  for (int i = threadIdx.x; i < npair; i += kCEThreads) {
    const float2 f = ld_bf2(x + 2 * i);
    const float mx = fmaxf(f.x, f.y);
    const float mz = mx == -INFINITY ? 0.f : mx;  // both masked: as in lm_ce_fwd_kernel
    online_merge(m, s, mx, __expf(f.x - mz) + __expf(f.y - mz));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    online_merge(m, s, m2, s2);
  }
  __shared__ float sm[kCEThreads / 64], ss[kCEThreads / 64];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sm[w] = m;
    ss[w] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0], S = ss[0];
    for (int k = 1; k < kCEThreads / 64; ++k) online_merge(M, S, sm[k], ss[k]);
    const float lse = M + logf(S);
    lse_out[row] = lse;
    row_loss[row] = lse - bf2f(x[lab]);
  }
}

__global__ void __launch_bounds__(kCEThreads)
ce_bwd_kernel(const bf16_t* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ lse,
              const float* __restrict__ scale_ptr, int V, int64_t ignore_index, bf16_t* __restrict__ dlogits) {
  const int64_t row = blockIdx.x;
  const int64_t lab = labels[row];
  const bool valid = !(lab == ignore_index || lab < 0 || lab >= V);
  const bf16_t* x = logits + row * V;
  uint32_t* dx = reinterpret_cast<uint32_t*>(dlogits + row * V);
  const int npair = V / 2;
  if (!valid) {
    for (int i = threadIdx.x; i < npair; i += kCEThreads) dx[i] = 0u;
    return;
  }
  const float scale = *scale_ptr, L = lse[row];
  for (int i = threadIdx.x; i < npair; i += kCEThreads) {
    const float2 f = ld_bf2(x + 2 * i);
    float g0 = __expf(f.x - L), g1 = __expf(f.y - L);
    if (2 * i == lab) g0 -= 1.f;
    if (2 * i + 1 == lab) g1 -= 1.f;
    const bfv2 q = __builtin_convertvector((f2v{g0 * scale, g1 * scale}), bfv2);
    dx[i] = __builtin_bit_cast(uint32_t, q);
  }
}

// ---- bias gradient: out[n] = sum_m g[m, n] -----------------------------------------------
// Workgroup = 16 column lanes (8 columns each, one 16-byte load) x 16 row lanes; each
// workgroup sums a [rows_per_split, 128] slab; the finalize pass adds <= 32 partials/column.
constexpr int kBGCols = 128;
constexpr int kBGRowLanes = 16;

__global__ void __launch_bounds__(256)
bias_grad_partial_kernel(const bf16_t* __restrict__ g, int64_t M, int N, int64_t rows_per_split,
                         float* __restrict__ part) {
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int col = blockIdx.x * kBGCols + cl * 8;
  const int64_t r0 = blockIdx.y * rows_per_split;
  const int64_t r1 = min(M, r0 + rows_per_split);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (col < N) {
    for (int64_t r = r0 + rl; r < r1; r += kBGRowLanes) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(g + r * N + col);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += bf2f(v.v[j]);
    }
  }
  __shared__ float red[kBGRowLanes][kBGCols + 4];
#pragma unroll
  for (int j = 0; j < 8; ++j) red[rl][cl * 8 + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < kBGCols) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kBGRowLanes; ++k) s += red[k][threadIdx.x];
    const int gc = blockIdx.x * kBGCols + threadIdx.x;
    if (gc < N) part[static_cast<int64_t>(blockIdx.y) * N + gc] = s;
  }
}

// Column sums for an N that is even but not a multiple of 8 (rows only 4-byte aligned: BERT's
// 30522-word decoder): 64 column lanes x 2 columns (one 4-byte load each: 256 contiguous bytes per
// row per wave) x 4 row lanes, the same [splits, N] partial layout as bias_grad_partial_kernel.
__global__ void __launch_bounds__(256)
bias_grad_partial2_kernel(const bf16_t* __restrict__ g, int64_t M, int N, int64_t rows_per_split,
                          float* __restrict__ part) {
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = blockIdx.x * 128 + cl * 2;
  const int64_t r0 = blockIdx.y * rows_per_split;
  const int64_t r1 = min(M, r0 + rows_per_split);
  float a0 = 0.f, a1 = 0.f;
  if (col < N) {
#pragma unroll 4
    for (int64_t r = r0 + rl; r < r1; r += 4) {
      const uint32_t u = *reinterpret_cast<const uint32_t*>(g + r * N + col);
      a0 += __uint_as_float(u << 16);
      a1 += __uint_as_float(u & 0xFFFF0000u);
    }
  }
  __shared__ float red[4][129];
  red[rl][2 * cl] = a0;
  red[rl][2 * cl + 1] = a1;
  __syncthreads();
  if (threadIdx.x < 128) {
    const float sum = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    const int gc = blockIdx.x * 128 + threadIdx.x;
    if (gc < N) part[static_cast<int64_t>(blockIdx.y) * N + gc] = sum;
  }
}

constexpr float kGeluC = 0.7978845608028654f;  // sqrt(2 / pi)
constexpr float kGeluA = 0.044715f;

__device__ __forceinline__ float tanh_fast(float u) {
  // 1 - 2 / (exp(2u) + 1): exact limits at +-inf, fp32 accuracy well below bf16 rounding
  return 1.f - 2.f / (__expf(2.f * u) + 1.f);
}

constexpr float kInvSqrt2 = 0.7071067811865476f, kInvSqrt2Pi = 0.3989422804014327f;

// gelu(x) and gelu'(x): ERF = the exact form 0.5 x (1 + erf(x / sqrt 2)) (BERT's "gelu"),
// else the tanh approximation (GPT-2's "gelu_new")
template <bool ERF>
__device__ __forceinline__ float gelu_f(float x) {
  if (ERF) return 0.5f * x * (1.f + erff(x * kInvSqrt2));
  return 0.5f * x * (1.f + tanh_fast(kGeluC * (x + kGeluA * x * x * x)));
}

template <bool ERF>
__device__ __forceinline__ float gelu_d(float x) {
  if (ERF) return 0.5f * (1.f + erff(x * kInvSqrt2)) + x * kInvSqrt2Pi * __expf(-0.5f * x * x);
  const float t = tanh_fast(kGeluC * (x + kGeluA * x * x * x));
  return 0.5f * (1.f + t) + 0.5f * x * (1.f - t * t) * kGeluC * (1.f + 3.f * kGeluA * x * x);
}

template <bool ERF>
__global__ void __launch_bounds__(256)
gelu_fwd_kernel(const bf16_t* __restrict__ h, bf16_t* __restrict__ g, int64_t nvec) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < nvec; i += stride) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(h + i * 8);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      o.v[j] = f2bf(gelu_f<ERF>(bf2f(v.v[j])));
    }
    *reinterpret_cast<bf16x8*>(g + i * 8) = o;
  }
}

// dh = gelu'(h) * dg (bf16 out) + fp32 column partials of dh: part[blockIdx.y][N]
template <bool ERF>
__global__ void __launch_bounds__(256)
gelu_bwd_bias_kernel(const bf16_t* __restrict__ dg, const bf16_t* __restrict__ h, bf16_t* __restrict__ dh, int64_t M,
                     int N, int64_t rows_per_split, float* __restrict__ part) {
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int col = blockIdx.x * kBGCols + cl * 8;
  const int64_t r0 = blockIdx.y * rows_per_split;
  const int64_t r1 = min(M, r0 + rows_per_split);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (col < N) {
    for (int64_t r = r0 + rl; r < r1; r += kBGRowLanes) {
      const int64_t off = r * N + col;
      const bf16x8 d = *reinterpret_cast<const bf16x8*>(dg + off);
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(h + off);
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o.v[j] = f2bf(gelu_d<ERF>(bf2f(v.v[j])) * bf2f(d.v[j]));
        acc[j] += bf2f(o.v[j]);  // the bias gradient sums the bf16 dh the weight GEMMs see
      }
      *reinterpret_cast<bf16x8*>(dh + off) = o;
    }
  }
  __shared__ float red[kBGRowLanes][kBGCols + 4];
#pragma unroll
  for (int j = 0; j < 8; ++j) red[rl][cl * 8 + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < kBGCols) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kBGRowLanes; ++k) s += red[k][threadIdx.x];
    const int gc = blockIdx.x * kBGCols + threadIdx.x;
    if (gc < N) part[static_cast<int64_t>(blockIdx.y) * N + gc] = s;
  }
}

// Batched conv-weight transforms for the input gradients (ops/conv.py _WeightXforms): one launch
// rewrites every registered layer's weights after an optimizer step.  Source: [K][C][R][S] bf16
// channels-last (memory [K][R][S][C]); destination: [C][K][Rp][Sp] channels-last (memory
// [C][Rp][Sp][K]) holding tap (rtap[rp], stap[sp]) -- mode 0: the 180-degree rotation
// (rtap[rp] = R - 1 - rp) the stride-1 dgrad convolves with; mode 1: the listed taps of one
// stride-2 phase sub-kernel.  Tiny tensors: a block row per layer, strided reads are fine.
struct XformDesc {  // 64 bytes: 8 int64 per row of the host table
  const bf16_t* src;
  bf16_t* dst;
  int64_t count;  // destination elements
  int K, C, R, S, Rp, Sp;
  int mode;
  int taps;  // mode 1: rtap[0] | rtap[1] << 8 | stap[0] << 16 | stap[1] << 24
  int pad_[2];
};
static_assert(sizeof(XformDesc) == 64, "XformDesc must match ops/conv.py's 8-int64 rows");

__global__ void __launch_bounds__(256) weight_xform_kernel(const XformDesc* __restrict__ descs) {
  const XformDesc d = descs[blockIdx.y];
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < d.count;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    const int k = static_cast<int>(i % d.K);
    int64_t t = i / d.K;
    const int sp = static_cast<int>(t % d.Sp);
    t /= d.Sp;
    const int rp = static_cast<int>(t % d.Rp);
    const int c = static_cast<int>(t / d.Rp);
    const int r = d.mode == 0 ? d.R - 1 - rp : (d.taps >> (8 * rp)) & 0xFF;
    const int s = d.mode == 0 ? d.S - 1 - sp : (d.taps >> (16 + 8 * sp)) & 0xFF;
    d.dst[i] = d.src[((static_cast<int64_t>(k) * d.R + r) * d.S + s) * d.C + c];
  }
}

// out[i] = sum_r part[r][i] (r = 0 .. W-1 in order: deterministic), cast to the output dtype: the
// split-K weight-gradient partials (ops/fused.py _weight_grad) -- few rows (W = 2..4) of millions
// of columns, so one thread per 4 columns (float4 loads, W loads in flight) instead of the
// many-row column-sum layout of the norm finalize (32 row lanes per column: 7/8 idle at W = 4).
template <bool BF16OUT>
__global__ void __launch_bounds__(256) sum_rows_kernel(const float* __restrict__ part, int W, int64_t H,
                                                       void* __restrict__ out) {
  const int64_t n4 = H >> 2;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n4;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    const float4* src = reinterpret_cast<const float4*>(part) + i;
    float4 a = src[0];
    for (int r = 1; r < W; ++r) {
      const float4 b = src[static_cast<int64_t>(r) * n4];
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    if (BF16OUT) Vec4<bf16_t>::st(static_cast<bf16_t*>(out) + 4 * i, a);
    else Vec4<float>::st(static_cast<float*>(out) + 4 * i, a);
  }
}

}  // namespace fused
}  // namespace damd

using namespace damd;
using namespace damd::fused;

// Occupancy probe: `nblk` workgroups of 256 threads that hold their CU slots for `usec`
// microseconds (wall clock), the footprint of a collective's kernel (one workgroup per channel)
// running next to the compute stream.  Used to measure how much the persistent conv kernels lose
// when a side-stream kernel takes CUs (scripts/dev/interference.py); not on any training path.
__global__ void __launch_bounds__(256) occupy_kernel(int64_t ticks, int* sink) {
  const int64_t t0 = wall_clock64();
  int spins = 0;
  while (wall_clock64() - t0 < ticks) {
    __builtin_amdgcn_s_sleep(8);
    ++spins;
  }
  if (spins < 0) sink[threadIdx.x] = spins;  // keeps the loop; never taken
}

extern "C" {

// descs: device array of n XformDesc (64 bytes each: ops/conv.py _WeightXforms builds the table)
void damd_weight_xform_launch(const void* descs, int n, int64_t max_count, hipStream_t st) {
  int64_t bx = (max_count + 255) / 256;
  if (bx > 64) bx = 64;
  DAMD_LAUNCH(weight_xform_kernel, dim3(static_cast<unsigned>(bx), static_cast<unsigned>(n)), dim3(256), 0, st,
              static_cast<const XformDesc*>(descs));
}

void damd_occupy_launch(int nblk, double usec, int* sink, hipStream_t st) {
  // wall_clock64 runs at 100 MHz on gfx950
  DAMD_LAUNCH(occupy_kernel, dim3(nblk), dim3(256), 0, st, static_cast<int64_t>(usec * 100.0), sink);
}

void damd_lm_ce_fwd_launch(const void* logits, const int64_t* labels, int64_t rows, int T, int V, int Vp,
                           int64_t ignore_index, float* row_loss, float* lse, hipStream_t st) {
  if (rows <= 0) return;
  DAMD_LAUNCH(lm_ce_fwd_kernel, dim3(static_cast<unsigned>(rows)), dim3(kCEThreads), 0, st,
                     static_cast<const bf16_t*>(logits), labels, T, V, Vp, ignore_index, row_loss, lse);
  DAMD_CHECK_LAUNCH();
}

void damd_lm_ce_bwd_launch(const void* logits, const int64_t* labels, const float* lse, const float* scale,
                           int64_t rows, int T, int V, int Vp, int64_t ignore_index, void* dlogits, hipStream_t st) {
  if (rows <= 0) return;
  DAMD_LAUNCH(lm_ce_bwd_kernel, dim3(static_cast<unsigned>(rows)), dim3(kCEThreads), 0, st,
                     static_cast<const bf16_t*>(logits), labels, lse, scale, T, V, Vp, ignore_index,
                     static_cast<bf16_t*>(dlogits));
  DAMD_CHECK_LAUNCH();
}

// rows x V bf16 logits (V even), labels [rows] int64
void damd_ce_fwd_launch(const void* logits, const int64_t* labels, int64_t rows, int V, int64_t ignore_index,
                        float* row_loss, float* lse, hipStream_t st) {
  if (rows <= 0) return;
  DAMD_LAUNCH(ce_fwd_kernel, dim3(static_cast<unsigned>(rows)), dim3(kCEThreads), 0, st,
              static_cast<const bf16_t*>(logits), labels, V, ignore_index, row_loss, lse);
}

void damd_ce_bwd_launch(const void* logits, const int64_t* labels, const float* lse, const float* scale, int64_t rows,
                        int V, int64_t ignore_index, void* dlogits, hipStream_t st) {
  if (rows <= 0) return;
  DAMD_LAUNCH(ce_bwd_kernel, dim3(static_cast<unsigned>(rows)), dim3(kCEThreads), 0, st,
              static_cast<const bf16_t*>(logits), labels, lse, scale, V, ignore_index, static_cast<bf16_t*>(dlogits));
}

int damd_bias_grad_splits(int64_t M, int N) {
  const int col_blocks = (N + kBGCols - 1) / kBGCols;
  int splits = static_cast<int>((1024 + col_blocks - 1) / col_blocks);  // ~1024 workgroups
  if (splits > 32) splits = 32;                                         // finalize adds <= 32
  const int64_t max_splits = (M + 127) / 128;                           // >= 128 rows per split
  if (splits > max_splits) splits = static_cast<int>(max_splits);
  return splits < 1 ? 1 : splits;
}

// Partial column sums [splits, N] (fp32); the host finishes with the wide column-sum pass
// of norm.hip (damd_norm_wgrad_finalize_launch), which writes the output dtype directly.
// (A single-launch "last block reduces" variant was measured 4-5x slower on MI355X: the
// agent-scope __threadfence each block needs before taking its ticket writes back the XCD's
// L2, so every block pays an L2 flush; the second ~5 us launch is far cheaper.)
void damd_bias_grad_launch(const void* g, int64_t M, int N, int splits, float* part, void* /*out*/,
                           int /*out_dtype*/, hipStream_t st) {
  if (M <= 0 || N <= 0) return;
  const int64_t rps = (M + splits - 1) / splits;
  dim3 grid((N + kBGCols - 1) / kBGCols, splits);
  if (N % 8 == 0)
    DAMD_LAUNCH(bias_grad_partial_kernel, grid, dim3(256), 0, st, static_cast<const bf16_t*>(g), M, N, rps, part);
  else  // N even: 4-byte aligned rows
    DAMD_LAUNCH(bias_grad_partial2_kernel, grid, dim3(256), 0, st, static_cast<const bf16_t*>(g), M, N, rps, part);
  DAMD_CHECK_LAUNCH();
}

// part: [W][H] fp32 (H % 4 == 0, 16-byte aligned), out: [H] bf16 (out_bf16) or fp32
void damd_sum_rows_launch(const float* part, int W, int64_t H, void* out, int out_bf16, hipStream_t st) {
  const int64_t n4 = H / 4;
  if (n4 <= 0 || W <= 0) return;
  const int64_t want = (n4 + 255) / 256;
  const dim3 grid(static_cast<unsigned>(want < 16384 ? want : 16384));
  if (out_bf16)
    DAMD_LAUNCH(sum_rows_kernel<true>, grid, dim3(256), 0, st, part, W, H, out);
  else
    DAMD_LAUNCH(sum_rows_kernel<false>, grid, dim3(256), 0, st, part, W, H, out);
  DAMD_CHECK_LAUNCH();
}

void damd_gelu_fwd_launch(const void* h, void* g, int64_t n, int exact, hipStream_t st) {
  const int64_t nvec = n / 8;
  if (nvec <= 0) return;
  const int64_t want = (nvec + 255) / 256;
  const dim3 grid(static_cast<unsigned>(want < 8192 ? want : 8192));
  if (exact)
    DAMD_LAUNCH(gelu_fwd_kernel<true>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(h), static_cast<bf16_t*>(g), nvec);
  else
    DAMD_LAUNCH(gelu_fwd_kernel<false>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(h), static_cast<bf16_t*>(g), nvec);
  DAMD_CHECK_LAUNCH();
}

// dh and bias-gradient partials [splits, N] (splits from damd_bias_grad_splits)
void damd_gelu_bwd_bias_launch(const void* dg, const void* h, void* dh, int64_t M, int N, int splits, float* part,
                               int exact, hipStream_t st) {
  if (M <= 0 || N <= 0) return;
  const int64_t rps = (M + splits - 1) / splits;
  dim3 grid((N + kBGCols - 1) / kBGCols, splits);
  if (exact)
    DAMD_LAUNCH(gelu_bwd_bias_kernel<true>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(dg),
                static_cast<const bf16_t*>(h), static_cast<bf16_t*>(dh), M, N, rps, part);
  else
    DAMD_LAUNCH(gelu_bwd_bias_kernel<false>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(dg),
                static_cast<const bf16_t*>(h), static_cast<bf16_t*>(dh), M, N, rps, part);
  DAMD_CHECK_LAUNCH();
}

}  // extern "C"

// ---- launch-check probe (tests/test_launch_check_gpu.py): fills `out` with 1.0 through a dynamic-LDS
// round trip; mode 0 = a valid launch, 1 = dynamic LDS far over the 160 KiB per-workgroup limit,
// 2 = a 2048-thread block (over the 1024-thread limit).  The invalid modes must raise, not return.
namespace damd {
__global__ void debug_fill_kernel(float* __restrict__ out, int n) {
  extern __shared__ float dbg_lds[];
  dbg_lds[threadIdx.x] = 1.f;
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = dbg_lds[threadIdx.x];
}
}  // namespace damd

extern "C" void damd_debug_launch(float* out, int n, int mode, hipStream_t st) {
  using namespace damd;
  const int threads = mode == 2 ? 2048 : 256;
  const size_t lds = mode == 1 ? (size_t{1} << 20) : threads * sizeof(float);
  DAMD_LAUNCH(debug_fill_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(threads), lds, st, out, n);
}
