// Flash-decoding attention for gfx950 / MI355X: a short query chunk at the END of a longer key /
// value sequence (generation against a KV cache).  bf16 in/out, fp32 accumulate, forward only.
//   q [B, H, Tq, D], k / v [B, Hkv, Tk, D], H % Hkv == 0, 1 <= Tq <= Tk, D in {64, 128};
//   query row i sits at absolute position p = Tk - Tq + i (bottom-right alignment);
//   causal: key j <= p; window W (with causal): also j >= p - W + 1; optional uint8 key mask.
//
// The problem is memory-bound -- R = (H / Hkv) * Tq <= 32 query rows against thousands of keys --
// so the design reads each K / V byte from HBM once per KV head and spreads the keys over the chip:
//
// Row packing.  The G = H / Hkv query heads of one KV head times the Tq chunk rows are the 16
//   columns of the S^T = K.Q^T MFMA (fragment layout: attention.hip); RT = 1 or 2 column tiles (a
//   template argument) serve R <= 16 / R <= 32.  Packed row rr = hg * Tq + i carries its own (head,
//   position): the causal / window bounds are two per-lane integers per column tile, the Q
//   fragments are loaded once and stay in registers, and every head of the group shares each K / V
//   load.
// Split over keys.  Grid (S, B * Hkv): workgroup s owns a contiguous range of the visited 64-key
//   tiles (tiles wholly below the window of the first query row are not visited).  K / V tiles have
//   no reuse across waves, so each of the 4 waves takes every 4th tile of the range and runs its own
//   online softmax -- no workgroup barrier in the loop.  K fragments (rows contiguous in D) come
//   straight from global memory into the A-operand registers; V needs the transposed operand and is
//   staged in a wave-private LDS slab (row stride D + 16), read with ds_read_b64_tr_b16.  The next
//   tile's V loads are issued before the S^T MFMAs and its K loads right after them (the K registers
//   are free by then), so both fly under the softmax and the O^T = V^T.P^T MFMAs.  The waves merge
//   (m, l, O) once, through the V slabs, after the loop.
// Partials.  S == 1: the merge writes bf16 o and the log-sum-exp.  S > 1: it writes fp32 partials
//   O [S, B, H, Tq, D] (unnormalised) and (m, l) [2, S, B, H, Tq]; attn_decode_combine_kernel
//   rescales and sums them in split order.  An empty or fully masked split / wave contributes
//   m = -inf, l = 0, O = 0.  A row with no attendable key gives zeros and lse = -inf.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no instantiation spills):
//   attn_decode_kernel<D, RT>    VGPRs (+AGPRs)  SGPRs  LDS bytes  waves / SIMD  scratch
//     <64, 1>                    152             69     41472      3             0
//     <64, 2>                    204             84     41984      2             0
//     <128, 1>                   240             69     74240      2             0
//     <128, 2>                   256 (+64)       84     74752      1             0
//   attn_decode_combine_kernel   25              35     0          8             0
//   The K and V tiles in flight (D / 2 VGPRs each) are most of the registers: a wave of the
//   memory-bound loop holds 16 KB (D = 64) or 32 KB (D = 128) of loads in flight per tile.
#include "common.h"
#include "attention_frag.h"

#include <math.h>

#include <stdlib.h>

namespace damd {
namespace attn {

struct DecodeArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o; float* lse;
  float* po; float* pml;  // S > 1: fp32 partials O [S][B][H][Tq][D], (m, l) [2][S][B][H][Tq]
  Strides sq, sk, sv, so;
  int B, H, G, Tq, Tk;
  int S, kt_begin, kt_end;  // key split; visited 64-key tiles [kt_begin, kt_end)
  int causal, window;       // window 0: none
  float scale_log2;         // softmax scale * log2(e)
  const uint8_t* km;        // [B][kms] key validity (nullptr: every key < Tk is valid)
  int64_t kms;
};

// K tile of a wave as MFMA A operands: lane (g, c) holds key k0 + nt * 16 + c, columns
// ds * 32 + 8 g .. + 7.  Keys >= Tk load zeros.
template <int D>
struct KFrag {
  s8 r[4][D / 32];
  __device__ __forceinline__ void load(const bf16_t* __restrict__ base, int64_t st, int k0, int Tk, int g, int c) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int key = k0 + nt * 16 + c;
#pragma unroll
      for (int ds = 0; ds < D / 32; ++ds) {
        s8 x = {0, 0, 0, 0, 0, 0, 0, 0};
        if (key < Tk) x = *reinterpret_cast<const s8*>(base + static_cast<int64_t>(key) * st + ds * 32 + 8 * g);
        r[nt][ds] = x;
      }
    }
  }
};

// V tile of a wave: 64 rows x D through the wave's 64 lanes (16-byte chunks, 64 / (D / 8) whole rows
// per load instruction), global -> registers -> the wave's row-major LDS slab.  Rows >= Tk are zeros
// (their probabilities are zero; the data must not be NaN).
template <int D>
struct VStage {
  static constexpr int CH = D / 8;
  s8 r[CH];
  __device__ __forceinline__ void load(const bf16_t* __restrict__ base, int64_t st, int k0, int Tk, int lane) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int idx = lane + i * 64, row = idx / CH, col = (idx % CH) * 8;
      s8 x = {0, 0, 0, 0, 0, 0, 0, 0};
      if (k0 + row < Tk) x = *reinterpret_cast<const s8*>(base + static_cast<int64_t>(k0 + row) * st + col);
      r[i] = x;
    }
  }
  __device__ __forceinline__ void store(bf16_t* img, int lane) const {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int idx = lane + i * 64, row = idx / CH, col = (idx % CH) * 8;
      *reinterpret_cast<s8*>(img + row * kLdsStride(D) + col) = r[i];
    }
  }
};

// LDS traffic of ONE wave on its own slab: the hardware runs a wave's LDS instructions in order, so
// only the compiler has to be kept from moving them across this point.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int D, int RT>
__global__ void __launch_bounds__(kThreads) attn_decode_kernel(DecodeArgs a) {
  constexpr int KP = kLdsStride(D), ROWS = 16 * RT;
  static_assert(ROWS * D * sizeof(float) <= kBlk * KP * sizeof(bf16_t), "the merge reuses the V slabs");
  __shared__ __attribute__((aligned(16))) bf16_t Vs[4][kBlk * KP];
  __shared__ float Ms[4][ROWS], Ls[4][ROWS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int s = blockIdx.x, bkv = blockIdx.y, Hkv = a.H / a.G, hkv = bkv % Hkv, b = bkv / Hkv;
  const int Tk = a.Tk, Tq = a.Tq, R = a.G * Tq;
  const bf16_t* Kp = a.k + b * a.sk.b + hkv * a.sk.h;
  const bf16_t* Vp = a.v + b * a.sv.b + hkv * a.sv.h;
  const uint8_t* KMp = a.km ? a.km + b * a.kms : nullptr;
  const int ntile = a.kt_end - a.kt_begin;
  const int t0 = a.kt_begin + static_cast<int>(static_cast<int64_t>(s) * ntile / a.S);
  const int t1 = a.kt_begin + static_cast<int>(static_cast<int64_t>(s + 1) * ntile / a.S);

  // the lane's packed row per column tile: Q fragments and the key range [kmin, kmax] of its position
  s8 qf[RT][D / 32];
  int kmin[RT], kmax[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int rr = rt * 16 + c, hg = rr / Tq, i = rr - hg * Tq, pos = Tk - Tq + i;
    const bool valid = rr < R;
    kmax[rt] = valid ? (a.causal ? pos : Tk - 1) : -1;  // a row past R attends nothing and is never written
    kmin[rt] = a.window > 0 ? pos - a.window + 1 : 0;
    const bf16_t* Qp = a.q + b * a.sq.b + (hkv * a.G + hg) * a.sq.h + static_cast<int64_t>(i) * a.sq.t;
#pragma unroll
    for (int ds = 0; ds < D / 32; ++ds) {
      s8 x = {0, 0, 0, 0, 0, 0, 0, 0};
      if (valid) x = *reinterpret_cast<const s8*>(Qp + ds * 32 + 8 * g);
      qf[rt][ds] = x;
    }
  }
  f4 oacc[RT][D / 16];
  float m[RT], l[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    m[rt] = -INFINITY;
    l[rt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) oacc[rt][dt] = f4{0.f, 0.f, 0.f, 0.f};
  }

  bf16_t* Vw = Vs[w];
  KFrag<D> kf;
  VStage<D> vs;
  if (t0 + w < t1) {
    kf.load(Kp, a.sk.t, (t0 + w) * kBlk, Tk, g, c);
    vs.load(Vp, a.sv.t, (t0 + w) * kBlk, Tk, lane);
  }
  for (int t = t0 + w; t < t1; t += 4) {
    const int k0 = t * kBlk;
    const bool more = t + 4 < t1;
    wave_lds_fence();  // the previous tile's transposed reads are issued
    vs.store(Vw, lane);
    wave_lds_fence();
    if (more) vs.load(Vp, a.sv.t, k0 + 4 * kBlk, Tk, lane);
    f4 sc[RT][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) sc[rt][nt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < D / 32; ++ds)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) sc[rt][nt] = mfma(kf.r[nt][ds], qf[rt][ds], sc[rt][nt]);
    }
    if (more) kf.load(Kp, a.sk.t, k0 + 4 * kBlk, Tk, g, c);
    // per-key validity of the lane's 16 keys (mask rows are padded to a multiple of 64 keys: the
    // word loads stay inside the row)
    uint32_t mw[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      mw[nt] = KMp ? *reinterpret_cast<const uint32_t*>(KMp + k0 + nt * 16 + 4 * g) : 0x01010101u;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      // raw scores; the softmax scale (> 0) is folded into the exp2 argument: p = 2^(s*c - m)
      float mx = -INFINITY;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + nt * 16 + 4 * g + r;
          const bool out = key > kmax[rt] || key < kmin[rt] || ((mw[nt] >> (8 * r)) & 0xffu) == 0;
          sc[rt][nt][r] = out ? -INFINITY : sc[rt][nt][r];
          mx = fmaxf(mx, sc[rt][nt][r]);
        }
      mx = rows_max(mx);
      const float m_new = fmaxf(m[rt], mx * a.scale_log2);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = ex2(m[rt] - m_use);
      float rs = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = ex2(fmaf(sc[rt][nt][r], a.scale_log2, -m_use));
          rs += p;
          sc[rt][nt][r] = p;
        }
      l[rt] = l[rt] * alpha + rs;
      m[rt] = m_new;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) oacc[rt][dt] *= alpha;
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      s8 pb[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) pb[rt] = pack_pair(sc[rt][2 * s2], sc[rt][2 * s2 + 1]);
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
        const s8 vf = tr_pair(Vw, KP, s2 * 32 + 4 * g, s2 * 32 + 16 + 4 * g, dt * 16, c);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) oacc[rt][dt] = mfma(vf, pb[rt], oacc[rt][dt]);
      }
    }
  }

  // merge the four waves: (m, l, O) of each wave into LDS (O over the wave's own V slab, row-major
  // [ROWS][D] fp32), then 16 / RT threads per packed row rescale and sum them
  wave_lds_fence();
  float* Ow = reinterpret_cast<float*>(Vw);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const float lt = rows_sum(l[rt]);
    if (g == 0) {
      Ms[w][rt * 16 + c] = m[rt];
      Ls[w][rt * 16 + c] = lt;
    }
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) *reinterpret_cast<f4*>(Ow + (rt * 16 + c) * D + dt * 16 + 4 * g) = oacc[rt][dt];
  }
  __syncthreads();
  constexpr int TPR = 16 / RT, CPT = D / TPR;  // threads per row, columns per thread
  const int rr = threadIdx.x / TPR, col0 = (threadIdx.x % TPR) * CPT;
  float M = -INFINITY;
#pragma unroll
  for (int ww = 0; ww < 4; ++ww) M = fmaxf(M, Ms[ww][rr]);
  const float Mu = M == -INFINITY ? 0.f : M;
  float L = 0.f;
  f4 acc[CPT / 4];
#pragma unroll
  for (int j = 0; j < CPT / 4; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ww = 0; ww < 4; ++ww) {
    const float f = ex2(Ms[ww][rr] - Mu);
    L += Ls[ww][rr] * f;
    const float* Op = reinterpret_cast<const float*>(Vs[ww]) + rr * D + col0;
#pragma unroll
    for (int j = 0; j < CPT / 4; ++j) acc[j] += *reinterpret_cast<const f4*>(Op + 4 * j) * f;
  }
  if (rr >= R) return;
  const int hg = rr / Tq, i = rr - hg * Tq, h = hkv * a.G + hg;
  if (a.S == 1) {
    const float inv = L > 0.f ? 1.f / L : 0.f;
    bf16_t* Op = a.o + b * a.so.b + h * a.so.h + static_cast<int64_t>(i) * a.so.t + col0;
#pragma unroll
    for (int j = 0; j < CPT / 4; ++j) {
      s4 ov;
#pragma unroll
      for (int r = 0; r < 4; ++r) ov[r] = bfs(acc[j][r] * inv);
      *reinterpret_cast<s4*>(Op + 4 * j) = ov;
    }
    if (col0 == 0) a.lse[(static_cast<int64_t>(b) * a.H + h) * Tq + i] = L > 0.f ? M * kLn2 + logf(L) : -INFINITY;
  } else {
    const int64_t rows = static_cast<int64_t>(a.B) * a.H * Tq;
    const int64_t row = s * rows + (static_cast<int64_t>(b) * a.H + h) * Tq + i;
    float* Pp = a.po + row * D + col0;
#pragma unroll
    for (int j = 0; j < CPT / 4; ++j) *reinterpret_cast<f4*>(Pp + 4 * j) = acc[j];
    if (col0 == 0) {
      a.pml[row] = M;
      a.pml[a.S * rows + row] = L;
    }
  }
}

// o = sum_s O_s 2^(m_s - M) / sum_s l_s 2^(m_s - M), M = max_s m_s, split 0 first (a fixed order: the
// same result for the same S on every run); lse = M ln 2 + log(sum).  One thread per 4 columns of a
// (batch, head, query) row; rows = B * H * Tq.
__global__ void __launch_bounds__(256) attn_decode_combine_kernel(const float* __restrict__ po,
                                                                  const float* __restrict__ pml, int S, bf16_t* o,
                                                                  Strides so, float* __restrict__ lse, int H, int Tq,
                                                                  int D, int64_t rows) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int vpr = D / 4;
  const int64_t row = idx / vpr;
  const int col = static_cast<int>(idx % vpr) * 4;
  if (row >= rows) return;
  float M = -INFINITY;
  for (int s = 0; s < S; ++s) M = fmaxf(M, pml[s * rows + row]);
  const float Mu = M == -INFINITY ? 0.f : M;
  float L = 0.f;
  f4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < S; ++s) {
    const float f = ex2(pml[s * rows + row] - Mu);
    L += pml[(S + s) * rows + row] * f;
    acc += *reinterpret_cast<const f4*>(po + (s * rows + row) * D + col) * f;
  }
  const int i = static_cast<int>(row % Tq);
  const int64_t bh = row / Tq;
  const int h = static_cast<int>(bh % H), b = static_cast<int>(bh / H);
  const float inv = L > 0.f ? 1.f / L : 0.f;
  s4 ov;
#pragma unroll
  for (int r = 0; r < 4; ++r) ov[r] = bfs(acc[r] * inv);
  *reinterpret_cast<s4*>(o + b * so.b + h * so.h + static_cast<int64_t>(i) * so.t + col) = ov;
  if (col == 0) lse[row] = L > 0.f ? M * kLn2 + logf(L) : -INFINITY;
}

}  // namespace attn
}  // namespace damd

using namespace damd;
using namespace damd::attn;

// The visited key tiles [begin, end) of a call: every tile up to the last key, from the tile that
// holds the lowest key in the window of the FIRST query row (position Tk - Tq) on.
static void decode_tiles(int Tq, int Tk, int window, int* begin, int* end) {
  const int lo = window > 0 ? Tk - Tq - window + 1 : 0;
  *begin = lo > 0 ? lo / kBlk : 0;
  *end = (Tk + kBlk - 1) / kBlk;
}

extern "C" {

// Workgroups per (batch, kv head): the key split S.  The unsplit grid is B * Hkv workgroups -- 8 for
// one Llama-8B sequence on a chip of 256 CUs -- so S grows until S * B * Hkv reaches two workgroups
// per CU (two fit: LDS 73 KB at D = 128), while every workgroup keeps at least 8 tiles: two per wave,
// so each wave's next-tile prefetch has a tile to hide behind.  Read off the forced-S sweep in
// profiles/attention_decode_probe.txt (Tq = 1, causal, call time): B8 Hkv8 D128 is flat between S = 4
// and 8 at Tk = 2048 .. 32768 and 1.4 - 2x slower unsplit; B1 Hkv8 Tk 8192 is fastest at S = 8 .. 16 (24 us)
// and loses 30% at S = 32, where a wave has one tile; past ~512 workgroups every shape slows down.
// DAMD_ATTN_DECODE_SPLIT=<S> forces it (clamped to [1, 256], NOT to the tile count: splits without a
// tile are legal and contribute nothing; read per launch: the tests switch it).
int damd_attn_decode_split(int B, int Hkv, int Tq, int Tk, int window) {
  const char* e = getenv("DAMD_ATTN_DECODE_SPLIT");
  const int forced = e ? atoi(e) : 0;
  if (forced >= 1) return forced < 256 ? forced : 256;
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    DAMD_CHECK(hipGetDevice(&dev));
    DAMD_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    cus = n > 0 ? n : 256;
  }
  int t0, t1;
  decode_tiles(Tq, Tk, window, &t0, &t1);
  const int64_t units = static_cast<int64_t>(B) * Hkv, cap = (t1 - t0) / 8;
  int64_t S = (2 * int64_t{cus} + units - 1) / units;
  if (S > cap) S = cap;
  if (S > 256) S = 256;
  return S < 1 ? 1 : static_cast<int>(S);
}

// The combine step on its own (attention_chunk.hip writes the same partials): po / pml as the kernels
// above leave them for `split` key splits, so: o's (b, h, t) strides in elements.
void damd_attn_decode_combine_launch(const float* po, const float* pml, int split, void* o, const int64_t* so,
                                     float* lse, int B, int H, int Tq, int D, hipStream_t st) {
  const int64_t rows = static_cast<int64_t>(B) * H * Tq, threads = rows * (D / 4);
  DAMD_LAUNCH(attn_decode_combine_kernel, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, st, po,
              pml, split, static_cast<bf16_t*>(o), Strides{so[0], so[1], so[2]}, lse, H, Tq, D, rows);
}

// strides: 4 tensors (q, k, v, o) x (b, h, t) in elements; km: optional [B][kms] key mask with
// kms >= pad64(Tk).  k, v have Hkv heads, H % Hkv == 0, (H / Hkv) * Tq <= 32, 1 <= Tq <= Tk (checked
// by the binding).  split > 1: po holds split * B * H * Tq * D floats, pml 2 * split * B * H * Tq.
void damd_attn_decode_launch(const void* q, const void* k, const void* v, void* o, float* lse, float* po, float* pml,
                             const int64_t* strides, int B, int H, int Hkv, int Tq, int Tk, int D, float scale,
                             int causal, int window, const uint8_t* km, int64_t kms, int split, hipStream_t st) {
  DecodeArgs a;
  a.q = static_cast<const bf16_t*>(q); a.k = static_cast<const bf16_t*>(k); a.v = static_cast<const bf16_t*>(v);
  a.o = static_cast<bf16_t*>(o); a.lse = lse; a.po = po; a.pml = pml;
  a.sq = {strides[0], strides[1], strides[2]}; a.sk = {strides[3], strides[4], strides[5]};
  a.sv = {strides[6], strides[7], strides[8]}; a.so = {strides[9], strides[10], strides[11]};
  a.B = B; a.H = H; a.G = H / Hkv; a.Tq = Tq; a.Tk = Tk;
  a.S = split;
  decode_tiles(Tq, Tk, window, &a.kt_begin, &a.kt_end);
  a.causal = causal; a.window = window; a.scale_log2 = scale * kLog2e;
  a.km = km; a.kms = kms;
  const dim3 grid(split, B * Hkv);
  const bool two = a.G * Tq > 16;
  if (D == 64) {
    if (two) DAMD_LAUNCH((attn_decode_kernel<64, 2>), grid, dim3(kThreads), 0, st, a);
    else DAMD_LAUNCH((attn_decode_kernel<64, 1>), grid, dim3(kThreads), 0, st, a);
  } else {
    if (two) DAMD_LAUNCH((attn_decode_kernel<128, 2>), grid, dim3(kThreads), 0, st, a);
    else DAMD_LAUNCH((attn_decode_kernel<128, 1>), grid, dim3(kThreads), 0, st, a);
  }
  if (split > 1) damd_attn_decode_combine_launch(po, pml, split, o, strides + 9, lse, B, H, Tq, D, st);
}

}  // extern "C"
