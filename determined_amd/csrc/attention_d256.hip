// Flash attention (forward + backward) at head dim 256 for gfx950 / MI355X: bf16 in/out, fp32
// accumulate, full / causal / band masks, optional key-padding mask, grouped-query K/V, no dropout.
// The Gemma-class shape: attention.hip's tiling (2 x 16 query rows x D accumulators per wave in the
// forward; K, V fragments and dK, dV accumulators of 16 keys x D in the dK/dV kernel) does not fit
// the register file at D = 256, so this file has its own.  Fragment layout, the S^T trick of the
// query-major kernels and the transposed LDS reads are those described at the top of attention.hip
// (helpers in attention_frag.h); argument layouts (strides, LSE, key mask, band arrays) are the same.
//
// Forward (workgroup = 4 waves = 64 query rows, a wave = ONE 16-row tile): the Q fragments (8 x s8)
//   and the 16 x 256 fp32 O^T accumulators (16 x f4) are 96 VGPRs before anything else, so the K/V
//   tile is kKT = 32 keys, not 64: the register-staged prefetch of the next tile is 32 VGPRs instead
//   of 64 and the S^T accumulators 8 instead of 16.  One tile is 16 MFMAs for S^T = K.Q^T (8 steps
//   of 32 over D per 16-key tile) and 16 for O^T += V^T.P^T (one permuted 32-key step per 16 columns
//   of D).  K and V (32 x 272 bf16 each, row stride D + 16: 544 B = 8 banks mod 64, the conflict-free
//   residue of the D = 128 tiles) take 34 KB of LDS.  Masking code runs only in tiles that need it (a
//   wave-uniform branch): ragged, diagonal, band-edge, or any tile under a key mask.
// dQ (same split; recomputes S^T and dP^T, no atomics): Q and dO fragments (64 VGPRs) + dQ^T
//   accumulators (64) + the 32-key S^T / dP^T pair (16) + the staged K/V prefetch (32).
// dK/dV (key-major, workgroup = 64 keys x HALF of D, a wave = 16 keys): S and dP need the whole head
//   dim, so the K and V fragments of the wave's keys stay in registers for all of D (64 VGPRs), but
//   the dK^T / dV^T accumulators cover 128 columns (2 x 8 x f4 = 64 VGPRs instead of 128), and two
//   workgroups -- on one XCD when B * Hkv is a multiple of 8: they read the same Q / dO blocks --
//   produce the two halves.  Cost: the S / dP MFMAs run twice (per 32 queries 32 + 32 MFMAs per half instead of
//   32 + 64 for the whole of D: 1.33x the MFMA work of an unsplit kernel), in exchange for no
//   accumulators in AGPRs, two waves per SIMD and twice the grid.  The query block is kQB = 32 rows
//   (Q and dO staged: 32 VGPRs, 34 KB of LDS).  One flat loop runs over (query head of the group,
//   query block) as in attention.hip's grouped-query kernel: the group sum happens in the
//   accumulators, so one kernel serves G = 1 and G > 1.  The head split of attention.hip
//   (damd_attn_gqa_split, fp32 partials) is left out, S = 1: the D split already doubles the grid.
// Band mode: tile skipping as in attention.hip at this file's granularity (32 keys / 32 queries).
//
// Registers and LDS (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; every kernel: no
// scratch, no spills, no AGPRs, 2 waves per SIMD; LDS per workgroup):
//   forward  full / causal / band: 200 / 202 / 188 VGPRs, 34816 B
//   dQ       full / causal / band: 238 / 240 / 224 VGPRs, 34816 B
//   dK/dV    full / causal / band: 230 / 240 / 242 VGPRs, 35072 B
// A 64-key tile (64-query block) adds 32 staging VGPRs to each: dQ and dK/dV would pass 256 and
// drop to one wave per SIMD, which is why the tiles are 32.
//
// Logit soft cap (template argument SOFTCAP, Gemma-2: y = c * tanh(s * scale / c) in place of s * scale):
// the raw score becomes t = tanh(.) = 1 - 2 / (1 + 2^(s * k1)) right after the S MFMAs (cap_tanh in
// attention_frag.h: one v_exp_f32 + one v_rcp_f32 per score) and c * log2(e) takes the place of the
// scale in the exp2 argument, so the cap precedes every mask select, the online maximum runs over
// capped values and the saved LSE is that of the capped logits.  The backward computes t, p and
// dS = p * (dP - delta) * (1 - t^2) per score in place (no array of t lives across the MFMAs); the
// final * scale of dQ / dK is unchanged.  SOFTCAP = true, same conditions (no scratch, no spills, no
// AGPRs, 2 waves per SIMD, same LDS):
//   forward  full / causal / band: 208 / 214 / 192 VGPRs
//   dQ       full / causal / band: 238 / 240 / 224 VGPRs
//   dK/dV    full / causal / band: 234 / 246 / 238 VGPRs

#include "common.h"
#include "attention_frag.h"

#include <math.h>

namespace damd {
namespace attn256 {

using namespace damd::attn;

constexpr int kD = 256;
constexpr int kKT = 32;             // keys per staged K/V tile (forward, dQ)
constexpr int kQB = 32;             // queries per staged Q/dO block (dK/dV)
constexpr int kRows = 64;           // query rows (forward, dQ) / keys (dK/dV) per workgroup
constexpr int kDH = kD / 2;         // columns of dK / dV per dK/dV workgroup
constexpr int kP = kLdsStride(kD);  // LDS row stride
constexpr int kFull = 0, kCausal = 1, kBand = 2;

struct Band {
  const int32_t* klo; const int32_t* khi;  // [b][query], rows padded to a multiple of 128 with empty ranges
  const int32_t* qlo; const int32_t* qhi;  // [b][key], likewise
  int64_t bs;                              // row stride (0: one row for every batch element)
};

struct Args {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; const bf16_t* dout;
  bf16_t* o; bf16_t* dq; bf16_t* dk; bf16_t* dv;
  float* lse; const float* delta;
  Strides sq, sk, sv, so, sdo, sdq, sdk, sdv;
  int H, T, G;  // G = H / Hkv query heads per K/V head
  float scale, scale_log2;
  float k1, k2;  // SOFTCAP (cap c): 2 * log2(e) * scale / c and c * log2(e); see cap_tanh
  const uint8_t* km;  // [B][kms] key validity, rows padded to a multiple of 64 (nullptr: every key < T is valid)
  int64_t kms;
  Band band;
};

// Band mode, rows [r0, r0 + 64) of a workgroup against tiles of `step` columns: the tiles
// [begin, end) hold every attended column -- the bounds are non-decreasing, so the first row has the
// lowest `lo` and the last valid row the highest `hi` -- and the columns [in_lo, in_hi) are attended
// by every row.  Clamped to the tiles that exist, whatever the arrays hold.  The query-major kernels
// pass (klo, khi), the key-major one (qlo, qhi).
struct Tiles {
  int begin, end, in_lo, in_hi;
};
__device__ __forceinline__ Tiles band_tiles(const int32_t* lo, const int32_t* hi, int r0, int step, int T) {
  const int rl = min(r0 + kRows, T) - 1, n = (T + step - 1) / step;
  Tiles t;
  t.begin = min(max(lo[r0], 0) / step, n);
  t.end = max(t.begin, (min(hi[rl], T) + step - 1) / step);
  t.in_lo = max(lo[rl], 0);
  t.in_hi = min(hi[r0], T);
  return t;
}

// Register-staged tile of 32 rows x 256 bf16 (4 x 16 bytes per thread): global -> registers (issued
// a tile ahead), registers -> row-major LDS image.  Rows >= T load zeros.
struct Stage {
  s8 r[4];
  __device__ __forceinline__ void load(const bf16_t* __restrict__ base, int64_t st, int r0, int T) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = threadIdx.x + i * kThreads, row = idx >> 5, col = (idx & 31) * 8;
      s8 x = {0, 0, 0, 0, 0, 0, 0, 0};
      if (r0 + row < T) x = *reinterpret_cast<const s8*>(base + static_cast<int64_t>(r0 + row) * st + col);
      r[i] = x;
    }
  }
  __device__ __forceinline__ void store(bf16_t* img) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = threadIdx.x + i * kThreads, row = idx >> 5, col = (idx & 31) * 8;
      *reinterpret_cast<s8*>(img + row * kP + col) = r[i];
    }
  }
};

// Workgroup -> (block j, unit): every block of one unit on ONE XCD (consecutive workgroup ids go
// round-robin to the 8 XCDs, each with its own L2), and the G units of a K/V group on the same XCD
// when there are a multiple of 8 groups; else the plain order.  attention.hip's map.
__device__ __forceinline__ void wg_map(int nblk, int G, int& j, int& u) {
  const int L = blockIdx.x, U = gridDim.x / nblk, UG = U / G;
  if ((UG & 7) == 0) {
    const int xcd = L & 7, slot = L >> 3, per = (UG >> 3) * G;
    j = slot / per;
    const int rem = slot - j * per, grp = rem / G;
    u = (grp * 8 + xcd) * G + (rem - grp * G);
  } else {
    j = L / U;
    u = L - j * U;
  }
}

// 16 query rows of a query-major wave: the lane's row (c) fragments of a [.., T, 256] tensor
__device__ __forceinline__ void load_rows(s8 (&f)[kD / 32], const bf16_t* p, int64_t st, int q, int g, int T) {
#pragma unroll
  for (int ds = 0; ds < kD / 32; ++ds) {
    s8 x = {0, 0, 0, 0, 0, 0, 0, 0};
    if (q < T) x = *reinterpret_cast<const s8*>(p + static_cast<int64_t>(q) * st + ds * 32 + 8 * g);
    f[ds] = x;
  }
}

// the lane's four accumulator rows of N 16-column tiles, scaled, as bf16 at row pointer p
template <int N>
__device__ __forceinline__ void store_rows(bf16_t* p, const f4 (&acc)[N], float mul, int g) {
#pragma unroll
  for (int dt = 0; dt < N; ++dt) {
    s4 ov;
#pragma unroll
    for (int r = 0; r < 4; ++r) ov[r] = bfs(acc[dt][r] * mul);
    *reinterpret_cast<s4*>(p + dt * 16 + 4 * g) = ov;
  }
}

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
template <int MODE, bool SOFTCAP>
__global__ void __launch_bounds__(kThreads) fwd_kernel(Args a) {
  constexpr bool CAUSAL = MODE == kCausal, BAND = MODE == kBand;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[kKT * kP];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[kKT * kP];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int T = a.T, nkb = (T + kKT - 1) / kKT, nqb = (T + kRows - 1) / kRows;
  int j, bhi;
  wg_map(nqb, a.G, j, bhi);
  const int qb = CAUSAL ? nqb - 1 - j : j;  // causal: the heaviest blocks are dispatched first
  const int h = bhi % a.H, b = bhi / a.H;
  const int q0 = qb * kRows, qw = q0 + w * 16, myq = qw + c;
  const bf16_t* Kp = a.k + b * a.sk.b + (h / a.G) * a.sk.h;
  const bf16_t* Vp = a.v + b * a.sv.b + (h / a.G) * a.sv.h;
  const uint8_t* KMp = a.km ? a.km + b * a.kms : nullptr;

  s8 qf[kD / 32];
  load_rows(qf, a.q + b * a.sq.b + h * a.sq.h, a.sq.t, myq, g, T);
  int klo = 0, khi = 0;  // band: the lane's key range (myq < padded row length)
  Tiles bt = {0, 0, 0, 0};
  if constexpr (BAND) {
    const int64_t row = b * a.band.bs;
    klo = a.band.klo[row + myq];
    khi = min(a.band.khi[row + myq], T);
    bt = band_tiles(a.band.klo + row, a.band.khi + row, q0, kKT, T);
  }
  f4 oacc[kD / 16];
#pragma unroll
  for (int dt = 0; dt < kD / 16; ++dt) oacc[dt] = f4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  const int kb_end = BAND ? bt.end : CAUSAL ? min(nkb, (q0 + kRows - 1) / kKT + 1) : nkb;
  const int kmax = CAUSAL ? min(T - 1, myq) : T - 1;
  Stage ks, vs;
  ks.load(Kp, a.sk.t, bt.begin * kKT, T);
  vs.load(Vp, a.sv.t, bt.begin * kKT, T);
  for (int kb = bt.begin; kb < kb_end; ++kb) {
    const int k0 = kb * kKT;
    __syncthreads();
    ks.store(Ks);
    vs.store(Vs);
    __syncthreads();
    if (kb + 1 < kb_end) {  // next tile's loads fly under this tile's MFMAs
      ks.load(Kp, a.sk.t, k0 + kKT, T);
      vs.load(Vp, a.sv.t, k0 + kKT, T);
    }
    f4 s[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int ds = 0; ds < kD / 32; ++ds)
        s[nt] = mfma(*reinterpret_cast<const s8*>(Ks + (nt * 16 + c) * kP + ds * 32 + 8 * g), qf[ds], s[nt]);
    // raw scores; the softmax scale (> 0) is folded into the exp2 argument: p = 2^(s*c - m).
    // SOFTCAP: s becomes tanh(s * scale / cap) BEFORE the mask (tanh(-inf) = -1 would un-mask a key)
    // and cap * log2(e) takes the place of the scale; the online maximum runs over the capped values.
    if constexpr (SOFTCAP) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[nt][r] = cap_tanh(s[nt][r] * a.k1);
    }
    const float sl = SOFTCAP ? a.k2 : a.scale_log2;
    const bool need_mask = k0 + kKT > T || (CAUSAL && k0 + kKT - 1 > qw) ||
                           (BAND && (k0 < bt.in_lo || k0 + kKT > bt.in_hi)) || KMp != nullptr;
    if (need_mask) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        // padded keys (rows padded to a multiple of 64: the word loads stay in bounds)
        const uint32_t mw = KMp ? *reinterpret_cast<const uint32_t*>(KMp + k0 + nt * 16 + 4 * g) : 0xffffffffu;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + nt * 16 + 4 * g + r;
          const bool out = (BAND ? (key < klo || key >= khi) : key > kmax) || !((mw >> (8 * r)) & 0xffu);
          s[nt][r] = out ? -INFINITY : s[nt][r];
        }
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[nt][r]);
    mx = rows_max(mx);
    const float m_new = fmaxf(m, mx * sl);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = ex2(m - m_use);
    float rs = 0.f;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[nt][r] = ex2(fmaf(s[nt][r], sl, -m_use));
        rs += s[nt][r];
      }
    l = l * alpha + rs;
    m = m_new;
    const s8 pb = pack_pair(s[0], s[1]);
#pragma unroll
    for (int dt = 0; dt < kD / 16; ++dt)
      oacc[dt] = mfma(tr_pair(Vs, kP, 4 * g, 16 + 4 * g, dt * 16, c), pb, oacc[dt] * alpha);
  }
  const float lt = rows_sum(l);
  if (myq < T) {
    store_rows(a.o + b * a.so.b + h * a.so.h + static_cast<int64_t>(myq) * a.so.t, oacc,
               lt > 0.f ? 1.f / lt : 0.f, g);
    if (g == 0) a.lse[(static_cast<int64_t>(b) * a.H + h) * T + myq] = lt > 0.f ? m * kLn2 + logf(lt) : -INFINITY;
  }
}

// ------------------------------------------------------------------------------------------
// dQ: query-major like the forward; S^T = K.Q^T, dP^T = V.dO^T, dS^T = P^T.(dP^T - delta),
// dQ^T += K^T.dS^T, written once as bf16
// ------------------------------------------------------------------------------------------
template <int MODE, bool SOFTCAP>
__global__ void __launch_bounds__(kThreads) dq_kernel(Args a) {
  constexpr bool CAUSAL = MODE == kCausal, BAND = MODE == kBand;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[kKT * kP];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[kKT * kP];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int T = a.T, nkb = (T + kKT - 1) / kKT, nqb = (T + kRows - 1) / kRows;
  int j, bhi;
  wg_map(nqb, a.G, j, bhi);
  const int qb = CAUSAL ? nqb - 1 - j : j;
  const int h = bhi % a.H, b = bhi / a.H;
  const int q0 = qb * kRows, qw = q0 + w * 16, myq = qw + c;
  const int64_t bh = static_cast<int64_t>(b) * a.H + h;
  const bf16_t* Kp = a.k + b * a.sk.b + (h / a.G) * a.sk.h;
  const bf16_t* Vp = a.v + b * a.sv.b + (h / a.G) * a.sv.h;
  const uint8_t* KMp = a.km ? a.km + b * a.kms : nullptr;

  s8 qf[kD / 32], of[kD / 32];
  load_rows(qf, a.q + b * a.sq.b + h * a.sq.h, a.sq.t, myq, g, T);
  load_rows(of, a.dout + b * a.sdo.b + h * a.sdo.h, a.sdo.t, myq, g, T);
  const float lse2 = myq < T ? a.lse[bh * T + myq] * kLog2e : INFINITY;
  const float dl = myq < T ? a.delta[bh * T + myq] : 0.f;
  int klo = 0, khi = 0;
  Tiles bt = {0, 0, 0, 0};
  if constexpr (BAND) {
    const int64_t row = b * a.band.bs;
    klo = a.band.klo[row + myq];
    khi = min(a.band.khi[row + myq], T);
    bt = band_tiles(a.band.klo + row, a.band.khi + row, q0, kKT, T);
  }
  f4 dq[kD / 16];
#pragma unroll
  for (int dt = 0; dt < kD / 16; ++dt) dq[dt] = f4{0.f, 0.f, 0.f, 0.f};

  const int kb_end = BAND ? bt.end : CAUSAL ? min(nkb, (q0 + kRows - 1) / kKT + 1) : nkb;
  const int kmax = CAUSAL ? min(T - 1, myq) : T - 1;
  Stage ks, vs;
  ks.load(Kp, a.sk.t, bt.begin * kKT, T);
  vs.load(Vp, a.sv.t, bt.begin * kKT, T);
  for (int kb = bt.begin; kb < kb_end; ++kb) {
    const int k0 = kb * kKT;
    __syncthreads();
    ks.store(Ks);
    vs.store(Vs);
    __syncthreads();
    if (kb + 1 < kb_end) {
      ks.load(Kp, a.sk.t, k0 + kKT, T);
      vs.load(Vp, a.sv.t, k0 + kKT, T);
    }
    f4 s[2], dp[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      s[nt] = dp[nt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < kD / 32; ++ds) {
        s[nt] = mfma(*reinterpret_cast<const s8*>(Ks + (nt * 16 + c) * kP + ds * 32 + 8 * g), qf[ds], s[nt]);
        dp[nt] = mfma(*reinterpret_cast<const s8*>(Vs + (nt * 16 + c) * kP + ds * 32 + 8 * g), of[ds], dp[nt]);
      }
    }
    const bool need_mask = k0 + kKT > T || (CAUSAL && k0 + kKT - 1 > qw) ||
                           (BAND && (k0 < bt.in_lo || k0 + kKT > bt.in_hi)) || KMp != nullptr;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const uint32_t mw = KMp ? *reinterpret_cast<const uint32_t*>(KMp + k0 + nt * 16 + 4 * g) : 0xffffffffu;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + nt * 16 + 4 * g + r;
        float x = s[nt][r], dcap = 1.f;  // SOFTCAP: x = tanh, dcap = 1 - tanh^2, per score in place
        if constexpr (SOFTCAP) x = cap_tanh(x * a.k1, dcap);
        float p = ex2(fmaf(x, SOFTCAP ? a.k2 : a.scale_log2, -lse2));
        if (need_mask)
          p = ((BAND ? (key < klo || key >= khi) : key > kmax) || !((mw >> (8 * r)) & 0xffu)) ? 0.f : p;
        s[nt][r] = SOFTCAP ? p * (dp[nt][r] - dl) * dcap : p * (dp[nt][r] - dl);  // dS^T
      }
    }
    const s8 sb = pack_pair(s[0], s[1]);
#pragma unroll
    for (int dt = 0; dt < kD / 16; ++dt) dq[dt] = mfma(tr_pair(Ks, kP, 4 * g, 16 + 4 * g, dt * 16, c), sb, dq[dt]);
  }
  if (myq < T)
    store_rows(a.dq + b * a.sdq.b + h * a.sdq.h + static_cast<int64_t>(myq) * a.sdq.t, dq, a.scale, g);
}

// ------------------------------------------------------------------------------------------
// dK/dV: 64 keys of one (batch, kv head) x one half of D per workgroup, summed over the group's
// heads in the accumulators
// ------------------------------------------------------------------------------------------
template <int MODE, bool SOFTCAP>
__global__ void __launch_bounds__(kThreads) dkv_kernel(Args a) {
  constexpr bool CAUSAL = MODE == kCausal, BAND = MODE == kBand;
  __shared__ __attribute__((aligned(16))) bf16_t Qs[kQB * kP];
  __shared__ __attribute__((aligned(16))) bf16_t dOs[kQB * kP];
  __shared__ float lse2[kQB], dl[kQB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int T = a.T, nkb = (T + kRows - 1) / kRows, nqb = (T + kQB - 1) / kQB, Hkv = a.H / a.G;
  int kb, unit;
  wg_map(nkb, 2, kb, unit);  // unit = (b*Hkv + hkv)*2 + half: both halves read the same Q / dO blocks
  const int col0 = (unit & 1) * kDH, bkv = unit >> 1;
  const int hkv = bkv % Hkv, b = bkv / Hkv;
  const int k0 = kb * kRows, mykey = k0 + w * 16 + c;
  const bf16_t* Qb = a.q + b * a.sq.b;
  const bf16_t* dOb = a.dout + b * a.sdo.b;
  const uint8_t* KMp = a.km ? a.km + b * a.kms : nullptr;
  const bool kvalid = mykey < T && (KMp == nullptr || KMp[mykey] != 0);

  s8 kf[kD / 32], vf[kD / 32];
  load_rows(kf, a.k + b * a.sk.b + hkv * a.sk.h, a.sk.t, mykey, g, T);
  load_rows(vf, a.v + b * a.sv.b + hkv * a.sv.h, a.sv.t, mykey, g, T);
  f4 dk[kDH / 16], dv[kDH / 16];
#pragma unroll
  for (int dt = 0; dt < kDH / 16; ++dt) dk[dt] = dv[dt] = f4{0.f, 0.f, 0.f, 0.f};

  // band: the lane's query range (mykey < padded row length), one block range for every head of the group
  Tiles kr = {0, 0, 0, 0};
  int qlo = 0, qhi = 0;
  if constexpr (BAND) {
    const int64_t row = b * a.band.bs;
    kr = band_tiles(a.band.qlo + row, a.band.qhi + row, k0, kQB, T);
    qlo = a.band.qlo[row + mykey];
    qhi = a.band.qhi[row + mykey];
  }
  const int qb0 = BAND ? kr.begin : CAUSAL ? k0 / kQB : 0, qb_end = BAND ? kr.end : nqb;
  const int h_end = (hkv + 1) * a.G;
  int h = qb0 >= qb_end ? h_end : hkv * a.G;  // query head of the iteration (no block: no iteration)
  Stage qst, ost;
  if (h < h_end) {
    qst.load(Qb + h * a.sq.h, a.sq.t, qb0 * kQB, T);
    ost.load(dOb + h * a.sdo.h, a.sdo.t, qb0 * kQB, T);
  }
  for (int qb = qb0; h < h_end;) {
    const int q0 = qb * kQB;
    const int64_t bh = static_cast<int64_t>(b) * a.H + h;
    __syncthreads();
    qst.store(Qs);
    ost.store(dOs);
    if (threadIdx.x < kQB) {
      const int q = q0 + threadIdx.x;
      lse2[threadIdx.x] = q < T ? a.lse[bh * T + q] * kLog2e : INFINITY;
      dl[threadIdx.x] = q < T ? a.delta[bh * T + q] : 0.f;
    }
    __syncthreads();
    // next iteration: the following query block, or the first block of the group's next head
    const bool last = qb + 1 == qb_end;
    const int nh = last ? h + 1 : h, nqb2 = last ? qb0 : qb + 1;
    if (nh < h_end) {
      qst.load(Qb + nh * a.sq.h, a.sq.t, nqb2 * kQB, T);
      ost.load(dOb + nh * a.sdo.h, a.sdo.t, nqb2 * kQB, T);
    }
    const bool need_mask = k0 + kRows > T || (CAUSAL && q0 < k0 + kRows) || KMp != nullptr ||
                           (BAND && (q0 < kr.in_lo || q0 + kQB > kr.in_hi));
    // S = Q.K^T and dP = dO.V^T over the whole head dim, the key on the lane
    f4 P[2], dS[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      f4 sacc = {0.f, 0.f, 0.f, 0.f}, dpacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < kD / 32; ++ds) {
        sacc = mfma(*reinterpret_cast<const s8*>(Qs + (qt * 16 + c) * kP + ds * 32 + 8 * g), kf[ds], sacc);
        dpacc = mfma(*reinterpret_cast<const s8*>(dOs + (qt * 16 + c) * kP + ds * 32 + 8 * g), vf[ds], dpacc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ql = qt * 16 + 4 * g + r;
        float x = sacc[r], dcap = 1.f;  // SOFTCAP: x = tanh, dcap = 1 - tanh^2
        if constexpr (SOFTCAP) x = cap_tanh(x * a.k1, dcap);
        float p = ex2(fmaf(x, SOFTCAP ? a.k2 : a.scale_log2, -lse2[ql]));
        if (need_mask)
          p = (!kvalid || (CAUSAL && mykey > q0 + ql) || (BAND && (q0 + ql < qlo || q0 + ql >= qhi))) ? 0.f : p;
        P[qt][r] = p;
        dS[qt][r] = SOFTCAP ? p * (dpacc[r] - dl[ql]) * dcap : p * (dpacc[r] - dl[ql]);
      }
    }
    // this half's columns: dV^T += dO^T . P ; dK^T += Q^T . dS  (one permuted step of 32 queries)
    const s8 pb = pack_pair(P[0], P[1]), sb = pack_pair(dS[0], dS[1]);
#pragma unroll
    for (int dt = 0; dt < kDH / 16; ++dt) {
      dv[dt] = mfma(tr_pair(dOs, kP, 4 * g, 16 + 4 * g, col0 + dt * 16, c), pb, dv[dt]);
      dk[dt] = mfma(tr_pair(Qs, kP, 4 * g, 16 + 4 * g, col0 + dt * 16, c), sb, dk[dt]);
    }
    h = nh;
    qb = nqb2;
  }
  if (mykey < T) {
    store_rows(a.dk + b * a.sdk.b + hkv * a.sdk.h + static_cast<int64_t>(mykey) * a.sdk.t + col0, dk, a.scale,
               g);
    store_rows(a.dv + b * a.sdv.b + hkv * a.sdv.h + static_cast<int64_t>(mykey) * a.sdv.t + col0, dv, 1.f, g);
  }
}

}  // namespace attn256
}  // namespace damd

using namespace damd;
using namespace damd::attn256;

// rowsum(dO . O) of the backward: attention.hip's kernel, instantiated there for D = 256
extern "C" void damd_attn_delta256_launch(const void* o, const int64_t* so, const void* dout, const int64_t* sdo,
                                          float* delta, int B, int H, int T, hipStream_t st);

#define DAMD_ATTN256_DISPATCH_CAP(KERNEL, CAP, GRID, ARGS)                                                \
  do {                                                                                                   \
    if ((ARGS).band.klo != nullptr) DAMD_LAUNCH((KERNEL<kBand, CAP>), GRID, dim3(kThreads), 0, st, ARGS); \
    else if (causal) DAMD_LAUNCH((KERNEL<kCausal, CAP>), GRID, dim3(kThreads), 0, st, ARGS);             \
    else DAMD_LAUNCH((KERNEL<kFull, CAP>), GRID, dim3(kThreads), 0, st, ARGS);                           \
  } while (0)

// softcap > 0 (the binding checked >= 0 and finite) picks the SOFTCAP instantiation
#define DAMD_ATTN256_DISPATCH(KERNEL, GRID, ARGS)                         \
  do {                                                                    \
    if (softcap > 0.f) DAMD_ATTN256_DISPATCH_CAP(KERNEL, true, GRID, ARGS); \
    else DAMD_ATTN256_DISPATCH_CAP(KERNEL, false, GRID, ARGS);            \
  } while (0)

extern "C" {

// strides: 4 tensors (q, k, v, o) x (b, h, t) in elements; km: optional [B][kms] key mask; klo .. qhi:
// the band arrays (all four or none), rows of band_stride int32 (0: one shared row) padded to a
// multiple of 128 entries >= T.  k, v have Hkv heads, H % Hkv == 0 (checked by the binding).
// softcap: the logit cap c (0: none), scores become c * tanh(q.k * scale / c) before the masks.
void damd_attn256_fwd_launch(const void* q, const void* k, const void* v, void* o, float* lse, const int64_t* s, int B,
                             int H, int Hkv, int T, float scale, int causal, const uint8_t* km, int64_t kms,
                             hipStream_t st, const int32_t* klo, const int32_t* khi, const int32_t* qlo,
                             const int32_t* qhi, int64_t band_stride, float softcap) {
  Args a = {};
  a.k1 = cap_k1(scale, softcap); a.k2 = softcap * kLog2e;
  a.q = static_cast<const bf16_t*>(q); a.k = static_cast<const bf16_t*>(k); a.v = static_cast<const bf16_t*>(v);
  a.o = static_cast<bf16_t*>(o); a.lse = lse;
  a.sq = {s[0], s[1], s[2]}; a.sk = {s[3], s[4], s[5]}; a.sv = {s[6], s[7], s[8]}; a.so = {s[9], s[10], s[11]};
  a.H = H; a.T = T; a.G = H / Hkv; a.scale = scale; a.scale_log2 = scale * kLog2e;
  a.km = km; a.kms = kms;
  a.band = {klo, khi, qlo, qhi, band_stride};
  const dim3 grid(((T + kRows - 1) / kRows) * H * B);
  DAMD_ATTN256_DISPATCH(fwd_kernel, grid, a);
}

// strides: 8 tensors (q, k, v, o, dout, dk, dv, dq) x (b, h, t).  k, v, dk, dv have Hkv heads.
// delta: [B, H, T] floats of scratch.
void damd_attn256_bwd_launch(const void* q, const void* k, const void* v, const void* o, const void* dout,
                             float* lse, float* delta, void* dq, void* dk, void* dv, const int64_t* s, int B, int H,
                             int Hkv, int T, float scale, int causal, const uint8_t* km, int64_t kms, hipStream_t st,
                             const int32_t* klo, const int32_t* khi, const int32_t* qlo, const int32_t* qhi,
                             int64_t band_stride, float softcap) {
  damd_attn_delta256_launch(o, s + 9, dout, s + 12, delta, B, H, T, st);
  Args a = {};
  a.k1 = cap_k1(scale, softcap); a.k2 = softcap * kLog2e;
  a.q = static_cast<const bf16_t*>(q); a.k = static_cast<const bf16_t*>(k); a.v = static_cast<const bf16_t*>(v);
  a.dout = static_cast<const bf16_t*>(dout); a.lse = lse; a.delta = delta;
  a.dq = static_cast<bf16_t*>(dq); a.dk = static_cast<bf16_t*>(dk); a.dv = static_cast<bf16_t*>(dv);
  a.sq = {s[0], s[1], s[2]}; a.sk = {s[3], s[4], s[5]}; a.sv = {s[6], s[7], s[8]};
  a.sdo = {s[12], s[13], s[14]}; a.sdk = {s[15], s[16], s[17]}; a.sdv = {s[18], s[19], s[20]};
  a.sdq = {s[21], s[22], s[23]};
  a.H = H; a.T = T; a.G = H / Hkv; a.scale = scale; a.scale_log2 = scale * kLog2e;
  a.km = km; a.kms = kms;
  a.band = {klo, khi, qlo, qhi, band_stride};
  const int nblk = (T + kRows - 1) / kRows;
  const dim3 kgrid(nblk * Hkv * B * 2), qgrid(nblk * H * B);
  DAMD_ATTN256_DISPATCH(dkv_kernel, kgrid, a);
  DAMD_ATTN256_DISPATCH(dq_kernel, qgrid, a);
}

}  // extern "C"
