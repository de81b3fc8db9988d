// Flash attention (forward + backward) for gfx950 / MI355X: bf16 in/out, fp32 accumulate,
// online softmax, full / causal / band masks, head dim D in {64, 128}.
//
// MFMA: v_mfma_f32_16x16x32_bf16 (a 64-wide wave computes a 16x16 tile, K = 32).
//   A operand: lane l holds A[row l&15][k 8(l>>4)+j], B operand: B[k 8(l>>4)+j][col l&15],
//   C/D: C[row 4(l>>4)+r][col l&15], r = 0..3.
// Transposed operands come from the SAME row-major LDS tile through ds_read_b64_tr_b16
// (gfx950 hardware transpose read: per 16-lane group, lane 4q+p addresses row q, columns
// 4p..4p+3 of a 4x16 block and lane i receives column i of the 4 rows).
//
// Forward (workgroup = 4 waves = 128 query rows, a wave = 2 x 16 rows):
//   S^T = K.Q^T puts the query on the lane (col) and 4 keys per 16-key tile in the lane's
//   registers: the online-softmax row max / sum are in-lane + 2 xor shuffles, the running
//   (m, l) and the rescale of O are lane-local, and O^T = V^T.P^T consumes P^T straight from
//   the S^T accumulators: a 32-key MFMA step uses the k order key(g, j) = (j < 4 ? 4g + j :
//   16 + 4g + j - 4), and the V^T operand is read in that order with two transposed reads.
//   K/V tiles (64 keys) are staged in LDS once per workgroup; the next tile's global loads
//   are issued into registers before the current tile's MFMAs (latency hidden).
//
// Backward (workgroup = 64 keys, a wave = 16 keys; loop over 64-row query blocks):
//   S = Q.K^T and dP = dO.V^T with the key on the lane (K, V fragments of the wave's keys stay
//   in registers), P = exp2(S.scale.log2e - LSE.log2e), dS = P.(dP - delta); P / dS feed
//   dV^T = dO^T.P and dK^T = Q^T.dS directly (dO^T, Q^T by transposed reads of the row-major
//   tiles).
// dQ (separate kernel, query-major like the forward): S^T = K.Q^T and dP^T = V.dO^T, P^T from
//   the saved LSE, dS^T = P^T.(dP^T - delta), dQ^T += K^T.dS^T, written once as bf16.  Summing
//   dQ over key blocks with float atomics instead (one 64x64 fp32 tile per key/query block
//   pair: ~285 MB of atomic adds per GPT-2-medium layer at mb 8) ran at the chip's atomic rate
//   and made the backward atomic-bound; recomputing S and dP costs two extra MFMA tiles per
//   block pair and no atomics.
//
// Grouped-query attention (K / V with Hkv heads, G = H / Hkv query heads per K/V head): the
//   forward and dQ kernels index K / V by h / G and keep one group's workgroups on one XCD
//   (wg_map); dK/dV is attn_bwd_gqa_kernel, which sums the group's heads in its accumulators.
//
// Band mode (sliding windows, packed documents; the third mask mode next to full and causal):
//   query q attends the contiguous keys [klo[q], khi[q]), both bounds non-decreasing in q, so the
//   queries of key k are contiguous too, [qlo[k], qhi[k]) -- four int32 arrays per batch row (or one
//   shared row), padded to a multiple of 128 entries with empty ranges so tile-granular loads need
//   no bounds branch.  The query-major kernels (forward, dQ) visit only the key tiles between
//   klo[first row] / 64 and ceil(khi[last valid row] / 64) -- monotone bounds make these the minimum
//   and maximum -- with the K/V prefetch starting at the first visited tile; the key-major kernels
//   (dK/dV, grouped-query dK/dV: one range for every head of the group) visit only the query blocks
//   between qlo[first key] / 64 and ceil(qhi[last valid key] / 64): O(T * W) instead of O(T^2).
//   The element mask is two integer compares against the lane's own (lo, hi) registers, taken only
//   in tiles that are not interior to every row's (key's) range; at D = 64 the forward's interior
//   tiles run the maskless body between masked leading and trailing edge tiles.  Workgroups run in
//   natural order (band work per block is roughly even).  The key mask and dropout compose as in
//   causal mode: the dropout counter is (seed, b*H + h, q, k) whatever the mask mode.
//   Registers at D = 64 (band instantiations, no dropout / dropout; waves per SIMD): forward QT = 1
//   104 / 114 VGPRs (4), QT = 2 156 / 164 (3) -- the same occupancy as causal (three loop copies of
//   the tile body; choosing the body per tile inside ONE loop took 200 VGPRs, 2 waves); dQ QT = 1
//   118 / 120 (4), QT = 2 196 / 200 (2); dK/dV 134 / 136 (3), grouped-query dK/dV 142 / 148 (3).
//
// Logit soft cap (template argument SOFTCAP of the four kernels, instantiated with DROP = false only;
//   Gemma-2: y = c * tanh(s * scale / c) in place of s * scale): the raw score becomes t = tanh(.) =
//   1 - 2 / (1 + 2^(s * k1)) right after the S MFMAs (cap_tanh in attention_frag.h: one v_exp_f32 + one
//   v_rcp_f32 per score; 2^x = inf gives t = 1, never a NaN) and k2 = c * log2(e) takes the place of the
//   scale in the exp2 argument.  So the cap precedes every mask select (tanh(-inf) = -1 would un-mask a
//   key), the maskless tile bodies cap too, the online maximum runs over capped values (NOT the
//   constant c: exp(y - c) underflows for rows near -c) and the saved LSE is that of the capped logits.
//   Backward: dS = p * (dP - delta) * (1 - t^2), with t, p and dS computed per score in place; dV, delta
//   and the final * scale of dQ / dK are unchanged.
//   Registers (VGPRs, full / causal / band; waves per SIMD as the DROP = false, SOFTCAP = false twin
//   in brackets; no scratch, no spills, LDS unchanged: 20480-20992 B at D = 64, 36864-37376 B at 128):
//     forward D = 64  QT = 1: 110 / 110 / 104 (4), twin 112 / 108 / 104;  QT = 2: 160 / 160 / 155 (3), twin 154 / 156 / 156
//     forward D = 128 QT = 1: 162 / 164 / 160 (3), twin 162 / 164 / 164;  QT = 2: 250 / 252 / 240 (2), twin 250 / 252 / 240
//     dQ      D = 64  QT = 1: 124 / 126 / 120 (4), twin 122 / 124 / 118;  QT = 2: 194 / 198 / 212 (2), twin 194 / 198 / 196
//     dQ      D = 128 QT = 1: 188 / 190 / 176 (2), twin 188 / 190 / 176;  QT = 2 (only when forced: DAMD_ATTN_QT):
//                              256 + 31 / 36 / 44 AGPRs (1), twin 256 + 30 / 33 / 28 AGPRs (1)
//     dK/dV   D = 64: 136 / 117 / 134 (3 / 4 / 3), twin 138 / 116 / 134;  D = 128: 222 / 202 / 205 (2), twin 224 / 210 / 212
//     dK/dV grouped-query D = 64: 116 / 118 / 142 (4 / 4 / 3), twin 115 / 116 / 142;  D = 128: 205 / 217 / 220 (2), twin 208 / 224 / 226
//
// Strides are in elements for (batch, head, token); the head dimension must be contiguous.
//
// Key padding (BERT-style batches): an optional byte mask km[b][key] (row stride kms, rows padded to
// a multiple of 64 keys with zeros) removes keys from every query's softmax; with a mask every key
// tile takes the masked body.  Dropout on the attention probabilities: keep(b, h, q, k) is a
// counter-based hash of (seed, b*H + h, q, k) compared with a threshold, recomputed identically by
// the forward, the dK/dV and the dQ kernels (no mask tensor is stored); kept probabilities are
// scaled by 1 / (1 - p).  The row sums (l, LSE) use the undropped probabilities, so the backward's
// delta = rowsum(dO . O) and dS = P . (Z . dP / (1 - p) - delta) hold unchanged.

#include "common.h"
#include "attention_frag.h"

#include <math.h>

#include <stdlib.h>

#include <type_traits>

#define DAMD_COMMA ,

namespace damd {
namespace attn {

// 16-row query tiles per wave in the forward / dQ kernels (QT, a template argument): a workgroup
// covers 64 * QT query rows.  QT = 2 reuses each staged K/V tile for twice the MFMAs; QT = 1 halves
// the live accumulators (<= 128 VGPRs at D = 64: 4 waves per SIMD instead of 2-3) and doubles the
// grid -- the better choice for causal masks at small batch x heads, where the heaviest query block
// is the critical path.
constexpr int fwd_rows(int QT) { return 4 * 16 * QT; }

struct KeyMaskDrop {
  const uint8_t* km;   // [B][kms] key validity (nullptr: every key < T is valid)
  int64_t kms;
  uint32_t seed;       // dropout stream
  uint32_t thresh;     // drop when hash < thresh (0: no dropout)
  float inv_keep;      // 1 / (1 - p)
  const int64_t* seedp;  // device-side seed (read at run time: a graph-captured step draws a new one per replay)
};

__device__ __forceinline__ uint32_t md_seed(const KeyMaskDrop& md) {
  return md.seedp != nullptr ? static_cast<uint32_t>(*md.seedp) : md.seed;
}

// Mask mode of the four attention kernels (a template argument).  Band: query q attends the keys
// [klo[q], khi[q]) and key k is attended by the queries [qlo[k], qhi[k]) -- two descriptions of one
// staircase, both bounds non-decreasing (sliding windows, packed documents).
constexpr int kFull = 0, kCausal = 1, kBand = 2;

struct Band {
  const int32_t* klo; const int32_t* khi;  // [b][query], rows padded to a multiple of 128 with empty ranges
  const int32_t* qlo; const int32_t* qhi;  // [b][key], likewise
  int64_t bs;                              // row stride (0: one row for every batch element)
};

struct FwdArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o; float* lse;
  Strides sq, sk, sv, so;
  int H, T, G;  // G = H / Hkv query heads per K/V head
  float scale_log2;  // softmax scale * log2(e)
  KeyMaskDrop md;
  Band band;
  float k1, k2;  // SOFTCAP (cap c): 2 * log2(e) * scale / c and c * log2(e); see cap_tanh
};

struct BwdArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; const bf16_t* dout;
  const float* lse; const float* delta; float* dq_acc; bf16_t* dk; bf16_t* dv;
  Strides sq, sk, sv, sdo, sdk, sdv;
  int H, T;
  int G, S;          // grouped-query dK/dV: group size, workgroups per group (head split)
  float* part;       // S > 1: fp32 partials [2 (dk, dv)][S][B * Hkv][T][D]
  float scale, scale_log2;
  KeyMaskDrop md;
  Band band;
  float k1, k2;  // SOFTCAP: as in FwdArgs
};

// Key-tile range of a query-major workgroup (forward, dQ) in band mode, rows [q0, q0 + rows): the
// tiles [begin, end) hold every attended key -- the bounds are non-decreasing, so the first row has
// the lowest klo and the last valid row the highest khi -- and the tiles [full_lo, full_hi) lie
// inside every row's range (no masking needed).  Clamped to the tiles that exist, whatever the
// arrays hold.
struct KeyTiles {
  int begin, end, full_lo, full_hi;
};
__device__ __forceinline__ KeyTiles band_key_tiles(const int32_t* klo, const int32_t* khi, int q0, int rows, int T) {
  const int ql = min(q0 + rows, T) - 1, nkb = (T + kBlk - 1) / kBlk;
  const int lo_first = max(klo[q0], 0), lo_last = max(klo[ql], 0);
  const int hi_first = min(khi[q0], T), hi_last = min(khi[ql], T);
  KeyTiles t;
  t.begin = min(lo_first / kBlk, nkb);
  t.end = max(t.begin, (hi_last + kBlk - 1) / kBlk);
  t.full_lo = (lo_last + kBlk - 1) / kBlk;
  t.full_hi = hi_first / kBlk;
  return t;
}

// The same for a key-major workgroup (dK/dV) with the keys [k0, k0 + 64): the 64-row query blocks
// [begin, end) hold every query that attends one of its keys, and the queries [in_lo, in_hi)
// attend all of them.
struct QueryBlocks {
  int begin, end, in_lo, in_hi;
};
__device__ __forceinline__ QueryBlocks band_query_blocks(const int32_t* qlo, const int32_t* qhi, int k0, int T) {
  const int kl = min(k0 + kBlk, T) - 1, nblk = (T + kBlk - 1) / kBlk;
  QueryBlocks t;
  t.begin = min(max(qlo[k0], 0) / kBlk, nblk);
  t.end = max(t.begin, (min(qhi[kl], T) + kBlk - 1) / kBlk);
  t.in_lo = max(qlo[kl], 0);
  t.in_hi = min(qhi[k0], T);
  return t;
}

// dropout decision for (b*H + h, query, key): murmur3-style finalizer of the mixed counters
__device__ __forceinline__ bool drop_keep(uint32_t seed, uint32_t thresh, uint32_t bh, uint32_t q, uint32_t k) {
  uint32_t x = seed ^ (bh * 0x9E3779B1u) ^ (q * 0x85EBCA77u) ^ (k * 0xC2B2AE3Du);
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x >= thresh;
}

// Register-staged tile of `ROWS` x D bf16: global -> registers (issued early), registers ->
// row-major LDS image (row stride kLdsStride(D)).  Rows >= T load zeros.
template <int D, int ROWS>
struct Stage {
  static constexpr int CH = D / 8;
  static constexpr int N = ROWS * CH / kThreads;
  s8 r[N];
  __device__ __forceinline__ void load(const bf16_t* __restrict__ base, int64_t st, int r0, int T) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int idx = threadIdx.x + i * kThreads, row = idx / CH, col = (idx % CH) * 8;
      s8 x = {0, 0, 0, 0, 0, 0, 0, 0};
      if (r0 + row < T) x = *reinterpret_cast<const s8*>(base + static_cast<int64_t>(r0 + row) * st + col);
      r[i] = x;
    }
  }
  __device__ __forceinline__ void store(bf16_t* img) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int idx = threadIdx.x + i * kThreads, row = idx / CH, col = (idx % CH) * 8;
      *reinterpret_cast<s8*>(img + row * kLdsStride(D) + col) = r[i];
    }
  }
};

// Workgroup -> (j, bh): a 1-D grid of nblk x B*H workgroups with every block of one (batch, head)
// on ONE XCD.  The dispatcher deals consecutive workgroup ids round-robin to the 8 XCDs (each with
// its own 4 MB L2); with the natural order a head's K/V (or Q/dO) tiles were fetched by workgroups
// on all 8 XCDs -- from the Infinity Cache / HBM, at a latency the one-tile-ahead prefetch cannot
// cover.  j = 0 is the heaviest block under a causal mask (dispatched first across the chip).
// Grouped-query attention (G = H / Hkv > 1 query heads read one K/V head): the unit that stays on
// one XCD is the (batch, kv head) group -- its G heads x nblk workgroups all read the same K/V
// tiles, which the per-head map would pull into eight L2s.  Needs B*Hkv % 8 == 0, else the plain
// order.  G = 1 is the per-head map unchanged.  The gain of the grouped map over the per-head
// one for G > 1 is unmeasured: profiles/attention_gqa_probe.txt times the kernels with this map
// against the MHA kernels on repeated K/V, not one map against the other.
__device__ __forceinline__ void wg_map(int nblk, int G, int& j, int& bh) {
  const int L = blockIdx.x, BH = gridDim.x / nblk, BKV = BH / G;
  if ((BKV & 7) == 0) {
    const int xcd = L & 7, slot = L >> 3, per = (BKV >> 3) * G;  // (kv group, head) pairs per XCD
    j = slot / per;
    const int rem = slot - j * per, grp = rem / G;
    bh = (grp * 8 + xcd) * G + (rem - grp * G);
  } else {
    j = L / BH;
    bh = L - j * BH;
  }
}

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
template <int D, int kQT, int MODE, bool DROP, bool SOFTCAP>
__global__ void __launch_bounds__(kThreads) attn_fwd_kernel(FwdArgs a) {
  static_assert(!(DROP && SOFTCAP), "the soft cap is instantiated without dropout only");
  constexpr bool CAUSAL = MODE == kCausal, BAND = MODE == kBand;
  constexpr int kFwdRows = fwd_rows(kQT);
  constexpr int KP = kLdsStride(D);
  __shared__ __attribute__((aligned(16))) bf16_t Ks[kBlk * KP];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[kBlk * KP];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int T = a.T, nkb = (T + kBlk - 1) / kBlk, nqb = (T + kFwdRows - 1) / kFwdRows;
  int j, bhi;
  wg_map(nqb, a.G, j, bhi);
  const int qb = CAUSAL ? nqb - 1 - j : j;
  const int h = bhi % a.H, b = bhi / a.H;
  const int q0 = qb * kFwdRows, qw = q0 + w * 16 * kQT;  // first query row of this wave
  const bf16_t* Qp = a.q + b * a.sq.b + h * a.sq.h;
  const bf16_t* Kp = a.k + b * a.sk.b + (h / a.G) * a.sk.h;
  const bf16_t* Vp = a.v + b * a.sv.b + (h / a.G) * a.sv.h;
  const uint8_t* KMp = a.md.km ? a.md.km + b * a.md.kms : nullptr;
  const uint32_t bh32 = static_cast<uint32_t>(b * a.H + h);

  s8 qf[kQT][D / 32];
  int klo[kQT], khi[kQT];  // band: the lane's key range, one per 16-row tile
#pragma unroll
  for (int qt = 0; qt < kQT; ++qt) {
    const int q = qw + qt * 16 + c;
    if constexpr (BAND) {  // q < padded row length
      klo[qt] = a.band.klo[b * a.band.bs + q];
      khi[qt] = min(a.band.khi[b * a.band.bs + q], T);
    }
#pragma unroll
    for (int ds = 0; ds < D / 32; ++ds) {
      s8 x = {0, 0, 0, 0, 0, 0, 0, 0};
      if (q < T) x = *reinterpret_cast<const s8*>(Qp + static_cast<int64_t>(q) * a.sq.t + ds * 32 + 8 * g);
      qf[qt][ds] = x;
    }
  }
  f4 oacc[kQT][D / 16];
  float m[kQT], l[kQT];
#pragma unroll
  for (int qt = 0; qt < kQT; ++qt) {
    m[qt] = -INFINITY;
    l[qt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) oacc[qt][dt] = f4{0.f, 0.f, 0.f, 0.f};
  }

  KeyTiles bt = {0, 0, 0, 0};
  if constexpr (BAND) bt = band_key_tiles(a.band.klo + b * a.band.bs, a.band.khi + b * a.band.bs, q0, kFwdRows, T);
  const int kb_end = BAND ? bt.end : CAUSAL ? min(nkb, (q0 + kFwdRows - 1) / kBlk + 1) : nkb;
  Stage<D, kBlk> ks, vs;
  ks.load(Kp, a.sk.t, bt.begin * kBlk, T);
  vs.load(Vp, a.sv.t, bt.begin * kBlk, T);
  // Leading tiles that no row of the workgroup masks (all keys < T and <= q0) run a body
  // compiled without any masking code; only the <= 2 diagonal / ragged tiles carry the selects.
  // (D = 128: a single masked body -- the unmasked copy pushes it to 256 VGPRs, 1 wave / SIMD)
  const int kb_full = D == 64 && !KMp ? min(kb_end, CAUSAL ? min((q0 + 1) / kBlk, T / kBlk) : T / kBlk) : 0;
  auto tile = [&](int kb, auto masked) {
    constexpr bool MASK = decltype(masked)::value;
    const int k0 = kb * kBlk;
    __syncthreads();
    ks.store(Ks);
    vs.store(Vs);
    __syncthreads();
    if (kb + 1 < kb_end) {  // next tile's loads fly under this tile's MFMAs
      ks.load(Kp, a.sk.t, k0 + kBlk, T);
      vs.load(Vp, a.sv.t, k0 + kBlk, T);
    }
    f4 s[kQT][4];
#pragma unroll
    for (int qt = 0; qt < kQT; ++qt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) s[qt][nt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int ds = 0; ds < D / 32; ++ds) {
        const s8 kf = *reinterpret_cast<const s8*>(Ks + (nt * 16 + c) * KP + ds * 32 + 8 * g);
#pragma unroll
        for (int qt = 0; qt < kQT; ++qt) s[qt][nt] = mfma(kf, qf[qt][ds], s[qt][nt]);
      }
    }
#pragma unroll
    for (int qt = 0; qt < kQT; ++qt) {
      const int myq = qw + qt * 16 + c;
      // raw scores; the softmax scale (> 0) is folded into the exp2 argument: p = 2^(s*c - m).
      // SOFTCAP (masked and maskless bodies alike): s becomes tanh(s * scale / cap) BEFORE the mask
      // (tanh(-inf) = -1 would un-mask a key) and cap * log2(e) takes the place of the scale; the
      // online maximum runs over the capped values.
      if constexpr (SOFTCAP) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[qt][nt][r] = cap_tanh(s[qt][nt][r] * a.k1);
      }
      const float sl = SOFTCAP ? a.k2 : a.scale_log2;
      if constexpr (MASK) {
        const int kmax = CAUSAL ? min(T - 1, myq) : T - 1;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = k0 + nt * 16 + 4 * g + r;
            const bool out = BAND ? (key < klo[qt] || key >= khi[qt]) : key > kmax;
            s[qt][nt][r] = out ? -INFINITY : s[qt][nt][r];
          }
        if (KMp) {  // padded keys (row padded to a multiple of 64: the word loads stay in bounds)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const uint32_t mw = *reinterpret_cast<const uint32_t*>(KMp + k0 + nt * 16 + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) s[qt][nt][r] = ((mw >> (8 * r)) & 0xffu) ? s[qt][nt][r] : -INFINITY;
          }
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[qt][nt][r]);
      mx = rows_max(mx);
      const float m_new = fmaxf(m[qt], mx * sl);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = ex2(m[qt] - m_use);
      float rs = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = ex2(fmaf(s[qt][nt][r], sl, -m_use));
          rs += p;
          if constexpr (DROP)
            s[qt][nt][r] = drop_keep(md_seed(a.md), a.md.thresh, bh32, myq, k0 + nt * 16 + 4 * g + r) ? p : 0.f;
          else
            s[qt][nt][r] = p;
        }
      }
      l[qt] = l[qt] * alpha + rs;
      m[qt] = m_new;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) oacc[qt][dt] *= alpha;
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      s8 pb[kQT];
#pragma unroll
      for (int qt = 0; qt < kQT; ++qt) pb[qt] = pack_pair(s[qt][2 * s2], s[qt][2 * s2 + 1]);
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
        const s8 vf = tr_pair(Vs, KP, s2 * 32 + 4 * g, s2 * 32 + 16 + 4 * g, dt * 16, c);
#pragma unroll
        for (int qt = 0; qt < kQT; ++qt) oacc[qt][dt] = mfma(vf, pb[qt], oacc[qt][dt]);
      }
    }
  };
  if constexpr (BAND) {
    // band: masked edge tiles on both sides of the interior ones; at D = 64 without a key mask
    // the interior tiles take the maskless body
    int kb = bt.begin;
    if constexpr (D == 64) {
      if (!KMp) {
        for (const int e = min(bt.full_lo, kb_end); kb < e; ++kb) tile(kb, std::true_type{});
        for (const int e = min(bt.full_hi, kb_end); kb < e; ++kb) tile(kb, std::false_type{});
      }
    }
    for (; kb < kb_end; ++kb) tile(kb, std::true_type{});
  } else {
    int kb = 0;
    for (; kb < kb_full; ++kb) tile(kb, std::false_type{});
    for (; kb < kb_end; ++kb) tile(kb, std::true_type{});
  }
#pragma unroll
  for (int qt = 0; qt < kQT; ++qt) {
    const float lt = rows_sum(l[qt]);
    const int myq = qw + qt * 16 + c;
    if (myq < T) {
      const float inv = lt > 0.f ? (DROP ? a.md.inv_keep : 1.f) / lt : 0.f;
      bf16_t* Op = a.o + b * a.so.b + h * a.so.h + static_cast<int64_t>(myq) * a.so.t;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
        s4 ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) ov[r] = bfs(oacc[qt][dt][r] * inv);
        *reinterpret_cast<s4*>(Op + dt * 16 + 4 * g) = ov;
      }
      if (g == 0)
        a.lse[(static_cast<int64_t>(b) * a.H + h) * T + myq] = lt > 0.f ? m[qt] * kLn2 + logf(lt) : -INFINITY;
    }
  }
}

// ------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------
// delta[b,h,t] = sum_d dO * O  (D/8 lanes per row, one 16-byte chunk each)
template <int D>
__global__ void __launch_bounds__(256) attn_delta_kernel(const bf16_t* __restrict__ o, Strides so,
                                                         const bf16_t* __restrict__ dout, Strides sd,
                                                         float* __restrict__ delta, int H, int T, int64_t rows) {
  constexpr int L = D / 8;
  const int64_t row = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) / L;
  const int part = threadIdx.x % L;
  float acc = 0.f;
  if (row < rows) {
    const int t = static_cast<int>(row % T);
    const int64_t bh = row / T;
    const int h = static_cast<int>(bh % H), b = static_cast<int>(bh / H);
    const s8 x = *reinterpret_cast<const s8*>(o + b * so.b + h * so.h + t * so.t + part * 8);
    const s8 y = *reinterpret_cast<const s8*>(dout + b * sd.b + h * sd.h + t * sd.t + part * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += bf2f(static_cast<bf16_t>(x[j])) * bf2f(static_cast<bf16_t>(y[j]));
  }
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (row < rows && part == 0) delta[row] = acc;
}

// One 64-query block of the dK/dV pass for a wave's 16 keys: the block's Q / dO tiles and its
// lse (x log2 e) / delta rows are staged in LDS, the K / V fragments of the keys stay in registers,
// dk / dv accumulate.  bh = b*H + (query head): the dropout counter.  Band mode: [qlo, qhi) is the
// query range of the lane's key, and the block [q0, q0 + 64) is interior when it lies inside the
// range of every key of the workgroup (kr: see band_query_blocks).
template <int D, int MODE, bool DROP, bool SOFTCAP>
__device__ __forceinline__ void bwd_block(const BwdArgs& a, const bf16_t* Qs, const bf16_t* dOs, const float* lse2,
                                          const float* dl, const s8 (&kf)[D / 32], const s8 (&vf)[D / 32],
                                          f4 (&dk)[D / 16], f4 (&dv)[D / 16], uint32_t bh, int q0, int k0, int mykey,
                                          bool kvalid, bool has_km, int qlo, int qhi, const QueryBlocks& kr) {
  static_assert(!(DROP && SOFTCAP), "the soft cap is instantiated without dropout only");
  constexpr bool CAUSAL = MODE == kCausal, BAND = MODE == kBand;
  constexpr int RP = kLdsStride(D);
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int T = a.T;
  const bool need_mask = (k0 + kBlk > T) || (CAUSAL && q0 < k0 + kBlk) || has_km ||
                         (BAND && (q0 < kr.in_lo || q0 + kBlk > kr.in_hi));
  // two halves of 32 queries: S / dP -> P / dS of one half feed its dV / dK MFMAs right away
  // (half the live P / dS registers: <= 128 VGPRs at D = 64, 4 waves per SIMD)
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    f4 P[2], dS[2];
#pragma unroll
    for (int hq = 0; hq < 2; ++hq) {
      const int qt = 2 * s2 + hq;
      f4 sacc = {0.f, 0.f, 0.f, 0.f}, dpacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < D / 32; ++ds) {
        const s8 qa = *reinterpret_cast<const s8*>(Qs + (qt * 16 + c) * RP + ds * 32 + 8 * g);
        const s8 oa = *reinterpret_cast<const s8*>(dOs + (qt * 16 + c) * RP + ds * 32 + 8 * g);
        sacc = mfma(qa, kf[ds], sacc);
        dpacc = mfma(oa, vf[ds], dpacc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ql = qt * 16 + 4 * g + r;
        float x = sacc[r], dcap = 1.f;  // SOFTCAP: x = tanh, dcap = 1 - tanh^2, per score in place
        if constexpr (SOFTCAP) x = cap_tanh(x * a.k1, dcap);
        float p = ex2(fmaf(x, SOFTCAP ? a.k2 : a.scale_log2, -lse2[ql]));
        if (need_mask)
          p = (!kvalid || (CAUSAL && mykey > q0 + ql) || (BAND && (q0 + ql < qlo || q0 + ql >= qhi))) ? 0.f : p;
        if constexpr (DROP) {
          const bool keep = drop_keep(md_seed(a.md), a.md.thresh, bh, q0 + ql, mykey);
          P[hq][r] = keep ? p * a.md.inv_keep : 0.f;  // dV uses the dropped, rescaled probabilities
          dS[hq][r] = p * ((keep ? dpacc[r] * a.md.inv_keep : 0.f) - dl[ql]);
        } else {
          P[hq][r] = p;
          dS[hq][r] = SOFTCAP ? p * (dpacc[r] - dl[ql]) * dcap : p * (dpacc[r] - dl[ql]);
        }
      }
    }
    // dV^T += dO^T . P ; dK^T += Q^T . dS   (k = 32 queries per step, permuted order)
    const s8 pb = pack_pair(P[0], P[1]);
    const s8 sb = pack_pair(dS[0], dS[1]);
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      dv[dt] = mfma(tr_pair(dOs, RP, s2 * 32 + 4 * g, s2 * 32 + 16 + 4 * g, dt * 16, c), pb, dv[dt]);
      dk[dt] = mfma(tr_pair(Qs, RP, s2 * 32 + 4 * g, s2 * 32 + 16 + 4 * g, dt * 16, c), sb, dk[dt]);
    }
  }
}

template <int D, int MODE, bool DROP, bool SOFTCAP>
__global__ void __launch_bounds__(kThreads) attn_bwd_kernel(BwdArgs a) {
  constexpr bool CAUSAL = MODE == kCausal, BAND = MODE == kBand;
  constexpr int RP = kLdsStride(D);
  __shared__ __attribute__((aligned(16))) bf16_t Qs[kBlk * RP];
  __shared__ __attribute__((aligned(16))) bf16_t dOs[kBlk * RP];
  __shared__ float lse2[kBlk], dl[kBlk];

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int T = a.T, nblk = (T + kBlk - 1) / kBlk;
  int kb, bhi;
  wg_map(nblk, 1, kb, bhi);  // causal: the lowest key blocks see the most query blocks
  const int h = bhi % a.H, b = bhi / a.H;
  const int k0 = kb * kBlk;
  const bf16_t* Qp = a.q + b * a.sq.b + h * a.sq.h;
  const bf16_t* Kp = a.k + b * a.sk.b + h * a.sk.h;
  const bf16_t* Vp = a.v + b * a.sv.b + h * a.sv.h;
  const bf16_t* dOp = a.dout + b * a.sdo.b + h * a.sdo.h;
  const int64_t bh = static_cast<int64_t>(b) * a.H + h;
  const int mykey = k0 + w * 16 + c;
  const uint8_t* KMp = a.md.km ? a.md.km + b * a.md.kms : nullptr;
  const bool kvalid = mykey < T && (KMp == nullptr || KMp[mykey] != 0);

  s8 kf[D / 32], vf[D / 32];
#pragma unroll
  for (int ds = 0; ds < D / 32; ++ds) {
    s8 x = {0, 0, 0, 0, 0, 0, 0, 0}, y = x;
    if (mykey < T) {
      x = *reinterpret_cast<const s8*>(Kp + static_cast<int64_t>(mykey) * a.sk.t + ds * 32 + 8 * g);
      y = *reinterpret_cast<const s8*>(Vp + static_cast<int64_t>(mykey) * a.sv.t + ds * 32 + 8 * g);
    }
    kf[ds] = x;
    vf[ds] = y;
  }
  f4 dk[D / 16], dv[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) dk[dt] = dv[dt] = f4{0.f, 0.f, 0.f, 0.f};

  // band: the lane's query range (mykey < padded row length) and the workgroup's query blocks
  QueryBlocks kr = {0, 0, 0, 0};
  int qlo = 0, qhi = 0;
  if constexpr (BAND) {
    const int64_t row = b * a.band.bs;
    kr = band_query_blocks(a.band.qlo + row, a.band.qhi + row, k0, T);
    qlo = a.band.qlo[row + mykey];
    qhi = a.band.qhi[row + mykey];
  }
  const int qb0 = BAND ? kr.begin : CAUSAL ? kb : 0, qb_end = BAND ? kr.end : nblk;
  Stage<D, kBlk> qst, ost;
  qst.load(Qp, a.sq.t, qb0 * kBlk, T);
  ost.load(dOp, a.sdo.t, qb0 * kBlk, T);
  for (int qb = qb0; qb < qb_end; ++qb) {
    const int q0 = qb * kBlk;
    __syncthreads();
    qst.store(Qs);
    ost.store(dOs);
    if (threadIdx.x < kBlk) {
      const int q = q0 + threadIdx.x;
      lse2[threadIdx.x] = q < T ? a.lse[bh * T + q] * kLog2e : INFINITY;
      dl[threadIdx.x] = q < T ? a.delta[bh * T + q] : 0.f;
    }
    __syncthreads();
    if (qb + 1 < qb_end) {
      qst.load(Qp, a.sq.t, q0 + kBlk, T);
      ost.load(dOp, a.sdo.t, q0 + kBlk, T);
    }

    bwd_block<D, MODE, DROP, SOFTCAP>(a, Qs, dOs, lse2, dl, kf, vf, dk, dv, static_cast<uint32_t>(bh), q0, k0, mykey, kvalid,
                             KMp != nullptr, qlo, qhi, kr);
  }
  if (mykey < T) {
    bf16_t* dKp = a.dk + b * a.sdk.b + h * a.sdk.h + static_cast<int64_t>(mykey) * a.sdk.t;
    bf16_t* dVp = a.dv + b * a.sdv.b + h * a.sdv.h + static_cast<int64_t>(mykey) * a.sdv.t;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      s4 kv, vv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        kv[r] = bfs(dk[dt][r] * a.scale);
        vv[r] = bfs(dv[dt][r]);
      }
      *reinterpret_cast<s4*>(dKp + dt * 16 + 4 * g) = kv;
      *reinterpret_cast<s4*>(dVp + dt * 16 + 4 * g) = vv;
    }
  }
}

// dK/dV of grouped-query attention (G = H / Hkv > 1).  A workgroup owns 64 keys of one (batch,
// kv head): its K / V fragments are loaded once, and ONE flat loop runs over (query head of the
// group, query block) with dk / dv accumulating in the same fp32 registers -- the group sum
// happens in the accumulators (no atomics, no [B, H, T, D] gradient, no reduction pass), and K / V
// are read once per group instead of once per query head.  The one-block-ahead Q / dO register
// prefetch runs across head boundaries: the loads of the next head's first block are issued
// before the MFMAs of the current head's last block, so the pipeline drains once, not G times.
// lse / delta / the dropout counter follow the query head of the iteration.
// Head split (a.S > 1, small grids): workgroup part s of S takes the heads [s*G/S, (s+1)*G/S) of
// the group (uneven when S does not divide G; S <= G, so no part is empty) and writes fp32
// partials a.part[dk|dv][s][b*Hkv + hkv][key][D]; attn_gqa_sum_kernel adds them in part order.
template <int D, int MODE, bool DROP, bool SOFTCAP>
__global__ void __launch_bounds__(kThreads) attn_bwd_gqa_kernel(BwdArgs a) {
  constexpr bool CAUSAL = MODE == kCausal, BAND = MODE == kBand;
  constexpr int RP = kLdsStride(D);
  __shared__ __attribute__((aligned(16))) bf16_t Qs[kBlk * RP];
  __shared__ __attribute__((aligned(16))) bf16_t dOs[kBlk * RP];
  __shared__ float lse2[kBlk], dl[kBlk];

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int T = a.T, nblk = (T + kBlk - 1) / kBlk, Hkv = a.H / a.G;
  int kb, unit;
  wg_map(nblk, 1, kb, unit);  // unit = (b*Hkv + hkv)*S + part: the blocks of one part share its heads' Q / dO
  const int part = unit % a.S, bkv = unit / a.S;
  const int hkv = bkv % Hkv, b = bkv / Hkv;
  const int hg0 = part * a.G / a.S, hg1 = (part + 1) * a.G / a.S;  // heads of the group, [hg0, hg1)
  const int k0 = kb * kBlk;
  const bf16_t* Qb = a.q + b * a.sq.b;
  const bf16_t* dOb = a.dout + b * a.sdo.b;
  const bf16_t* Kp = a.k + b * a.sk.b + hkv * a.sk.h;
  const bf16_t* Vp = a.v + b * a.sv.b + hkv * a.sv.h;
  const int mykey = k0 + w * 16 + c;
  const uint8_t* KMp = a.md.km ? a.md.km + b * a.md.kms : nullptr;
  const bool kvalid = mykey < T && (KMp == nullptr || KMp[mykey] != 0);

  s8 kf[D / 32], vf[D / 32];
#pragma unroll
  for (int ds = 0; ds < D / 32; ++ds) {
    s8 x = {0, 0, 0, 0, 0, 0, 0, 0}, y = x;
    if (mykey < T) {
      x = *reinterpret_cast<const s8*>(Kp + static_cast<int64_t>(mykey) * a.sk.t + ds * 32 + 8 * g);
      y = *reinterpret_cast<const s8*>(Vp + static_cast<int64_t>(mykey) * a.sv.t + ds * 32 + 8 * g);
    }
    kf[ds] = x;
    vf[ds] = y;
  }
  f4 dk[D / 16], dv[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) dk[dt] = dv[dt] = f4{0.f, 0.f, 0.f, 0.f};

  // band: one query-block range for every head of the group
  QueryBlocks kr = {0, 0, 0, 0};
  int qlo = 0, qhi = 0;
  if constexpr (BAND) {
    const int64_t row = b * a.band.bs;
    kr = band_query_blocks(a.band.qlo + row, a.band.qhi + row, k0, T);
    qlo = a.band.qlo[row + mykey];
    qhi = a.band.qhi[row + mykey];
  }
  const int qb0 = BAND ? kr.begin : CAUSAL ? kb : 0, qb_end = BAND ? kr.end : nblk;
  const int h_end = hkv * a.G + hg1;
  int h = BAND && qb0 >= qb_end ? h_end : hkv * a.G + hg0;  // query head of the iteration (band: no block, no iteration)
  Stage<D, kBlk> qst, ost;
  if (!BAND || h < h_end) {
    qst.load(Qb + h * a.sq.h, a.sq.t, qb0 * kBlk, T);
    ost.load(dOb + h * a.sdo.h, a.sdo.t, qb0 * kBlk, T);
  }
  for (int qb = qb0; h < h_end;) {
    const int q0 = qb * kBlk;
    const int64_t bh = static_cast<int64_t>(b) * a.H + h;
    __syncthreads();
    qst.store(Qs);
    ost.store(dOs);
    if (threadIdx.x < kBlk) {
      const int q = q0 + threadIdx.x;
      lse2[threadIdx.x] = q < T ? a.lse[bh * T + q] * kLog2e : INFINITY;
      dl[threadIdx.x] = q < T ? a.delta[bh * T + q] : 0.f;
    }
    __syncthreads();
    // next iteration: the following query block, or the first block of the next head
    const bool last = qb + 1 == qb_end;
    const int nh = last ? h + 1 : h, nqb = last ? qb0 : qb + 1;
    if (nh < h_end) {
      qst.load(Qb + nh * a.sq.h, a.sq.t, nqb * kBlk, T);
      ost.load(dOb + nh * a.sdo.h, a.sdo.t, nqb * kBlk, T);
    }
    bwd_block<D, MODE, DROP, SOFTCAP>(a, Qs, dOs, lse2, dl, kf, vf, dk, dv, static_cast<uint32_t>(bh), q0, k0, mykey, kvalid,
                             KMp != nullptr, qlo, qhi, kr);
    h = nh;
    qb = nqb;
  }
  if (mykey >= T) return;
  if (a.S == 1) {
    bf16_t* dKp = a.dk + b * a.sdk.b + hkv * a.sdk.h + static_cast<int64_t>(mykey) * a.sdk.t;
    bf16_t* dVp = a.dv + b * a.sdv.b + hkv * a.sdv.h + static_cast<int64_t>(mykey) * a.sdv.t;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      s4 kv, vv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        kv[r] = bfs(dk[dt][r] * a.scale);
        vv[r] = bfs(dv[dt][r]);
      }
      *reinterpret_cast<s4*>(dKp + dt * 16 + 4 * g) = kv;
      *reinterpret_cast<s4*>(dVp + dt * 16 + 4 * g) = vv;
    }
  } else {
    const int64_t plane = static_cast<int64_t>(gridDim.x / (nblk * a.S)) * T * D;  // B*Hkv*T*D
    float* pk = a.part + (part * plane + (static_cast<int64_t>(bkv) * T + mykey) * D);
    float* pv = pk + a.S * plane;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      *reinterpret_cast<f4*>(pk + dt * 16 + 4 * g) = dk[dt] * a.scale;
      *reinterpret_cast<f4*>(pv + dt * 16 + 4 * g) = dv[dt];
    }
  }
}

// dk / dv = sum over the S head-split partials, part 0 first (a fixed order: the same result for
// the same S on every run), written as bf16 through the dK / dV strides.  One thread per 4 columns.
__global__ void __launch_bounds__(256) attn_gqa_sum_kernel(const float* __restrict__ part, int S, bf16_t* dk, Strides sdk,
                                                           bf16_t* dv, Strides sdv, int Hkv, int T, int D,
                                                           int64_t plane) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * 4;
  if (i >= plane) return;
  f4 k = *reinterpret_cast<const f4*>(part + i), v = *reinterpret_cast<const f4*>(part + S * plane + i);
  for (int s = 1; s < S; ++s) {
    k += *reinterpret_cast<const f4*>(part + s * plane + i);
    v += *reinterpret_cast<const f4*>(part + (S + s) * plane + i);
  }
  const int d = static_cast<int>(i % D), t = static_cast<int>(i / D % T);
  const int64_t bkv = i / D / T;
  const int hkv = static_cast<int>(bkv % Hkv), b = static_cast<int>(bkv / Hkv);
  s4 kv, vv;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    kv[r] = bfs(k[r]);
    vv[r] = bfs(v[r]);
  }
  *reinterpret_cast<s4*>(dk + b * sdk.b + hkv * sdk.h + static_cast<int64_t>(t) * sdk.t + d) = kv;
  *reinterpret_cast<s4*>(dv + b * sdv.b + hkv * sdv.h + static_cast<int64_t>(t) * sdv.t + d) = vv;
}

struct DqArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; const bf16_t* dout;
  const float* lse; const float* delta; bf16_t* dq;
  Strides sq, sk, sv, sdo, sdq;
  int H, T, G;
  float scale, scale_log2;
  KeyMaskDrop md;
  Band band;
  float k1, k2;  // SOFTCAP: as in FwdArgs
};

// dQ for a block of kFwdRows query rows (same wave / lane layout as the forward).
template <int D, int kQT, int MODE, bool DROP, bool SOFTCAP>
__global__ void __launch_bounds__(kThreads) attn_dq_kernel(DqArgs a) {
  static_assert(!(DROP && SOFTCAP), "the soft cap is instantiated without dropout only");
  constexpr bool CAUSAL = MODE == kCausal, BAND = MODE == kBand;
  constexpr int kFwdRows = fwd_rows(kQT);
  constexpr int KP = kLdsStride(D);
  __shared__ __attribute__((aligned(16))) bf16_t Ks[kBlk * KP];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[kBlk * KP];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int T = a.T, nkb = (T + kBlk - 1) / kBlk, nqb = (T + kFwdRows - 1) / kFwdRows;
  int j, bhi;
  wg_map(nqb, a.G, j, bhi);
  const int qb = CAUSAL ? nqb - 1 - j : j;
  const int h = bhi % a.H, b = bhi / a.H;
  const int q0 = qb * kFwdRows, qw = q0 + w * 16 * kQT;
  const int64_t bh = static_cast<int64_t>(b) * a.H + h;
  const bf16_t* Qp = a.q + b * a.sq.b + h * a.sq.h;
  const bf16_t* Kp = a.k + b * a.sk.b + (h / a.G) * a.sk.h;
  const bf16_t* Vp = a.v + b * a.sv.b + (h / a.G) * a.sv.h;
  const bf16_t* dOp = a.dout + b * a.sdo.b + h * a.sdo.h;
  const uint8_t* KMp = a.md.km ? a.md.km + b * a.md.kms : nullptr;

  s8 qf[kQT][D / 32], of[kQT][D / 32];
  float lse2[kQT], dl[kQT];
  int klo[kQT], khi[kQT];  // band: the lane's key range, one per 16-row tile
#pragma unroll
  for (int qt = 0; qt < kQT; ++qt) {
    const int q = qw + qt * 16 + c;
    if constexpr (BAND) {  // q < padded row length
      klo[qt] = a.band.klo[b * a.band.bs + q];
      khi[qt] = min(a.band.khi[b * a.band.bs + q], T);
    }
#pragma unroll
    for (int ds = 0; ds < D / 32; ++ds) {
      s8 x = {0, 0, 0, 0, 0, 0, 0, 0}, y = x;
      if (q < T) {
        x = *reinterpret_cast<const s8*>(Qp + static_cast<int64_t>(q) * a.sq.t + ds * 32 + 8 * g);
        y = *reinterpret_cast<const s8*>(dOp + static_cast<int64_t>(q) * a.sdo.t + ds * 32 + 8 * g);
      }
      qf[qt][ds] = x;
      of[qt][ds] = y;
    }
    lse2[qt] = q < T ? a.lse[bh * T + q] * kLog2e : INFINITY;
    dl[qt] = q < T ? a.delta[bh * T + q] : 0.f;
  }
  f4 dq[kQT][D / 16];
#pragma unroll
  for (int qt = 0; qt < kQT; ++qt)
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) dq[qt][dt] = f4{0.f, 0.f, 0.f, 0.f};

  KeyTiles bt = {0, 0, 0, 0};
  if constexpr (BAND) bt = band_key_tiles(a.band.klo + b * a.band.bs, a.band.khi + b * a.band.bs, q0, kFwdRows, T);
  const int kb_end = BAND ? bt.end : CAUSAL ? min(nkb, (q0 + kFwdRows - 1) / kBlk + 1) : nkb;
  Stage<D, kBlk> ks, vs;
  ks.load(Kp, a.sk.t, bt.begin * kBlk, T);
  vs.load(Vp, a.sv.t, bt.begin * kBlk, T);
  for (int kb = bt.begin; kb < kb_end; ++kb) {
    const int k0 = kb * kBlk;
    __syncthreads();
    ks.store(Ks);
    vs.store(Vs);
    __syncthreads();
    if (kb + 1 < kb_end) {
      ks.load(Kp, a.sk.t, k0 + kBlk, T);
      vs.load(Vp, a.sv.t, k0 + kBlk, T);
    }
    // S^T = K.Q^T and dP^T = V.dO^T (key on the accumulator rows, query on the lane)
    f4 s[kQT][4], dp[kQT][4];
#pragma unroll
    for (int qt = 0; qt < kQT; ++qt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) s[qt][nt] = dp[qt][nt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int ds = 0; ds < D / 32; ++ds) {
        const s8 kf = *reinterpret_cast<const s8*>(Ks + (nt * 16 + c) * KP + ds * 32 + 8 * g);
        const s8 vf = *reinterpret_cast<const s8*>(Vs + (nt * 16 + c) * KP + ds * 32 + 8 * g);
#pragma unroll
        for (int qt = 0; qt < kQT; ++qt) {
          s[qt][nt] = mfma(kf, qf[qt][ds], s[qt][nt]);
          dp[qt][nt] = mfma(vf, of[qt][ds], dp[qt][nt]);
        }
      }
    }
    const bool need_mask = (k0 + kBlk > T) || (CAUSAL && k0 + kBlk - 1 > qw) ||
                           (BAND && (kb < bt.full_lo || kb >= bt.full_hi));
#pragma unroll
    for (int qt = 0; qt < kQT; ++qt) {
      const int myq = qw + qt * 16 + c;
      const int kmax = CAUSAL ? min(T - 1, myq) : T - 1;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const uint32_t mw = KMp ? *reinterpret_cast<const uint32_t*>(KMp + k0 + nt * 16 + 4 * g) : 0xffffffffu;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + nt * 16 + 4 * g + r;
          float x = s[qt][nt][r], dcap = 1.f;  // SOFTCAP: x = tanh, dcap = 1 - tanh^2
          if constexpr (SOFTCAP) x = cap_tanh(x * a.k1, dcap);
          float p = ex2(fmaf(x, SOFTCAP ? a.k2 : a.scale_log2, -lse2[qt]));
          if (need_mask) p = (BAND ? (key < klo[qt] || key >= khi[qt]) : key > kmax) ? 0.f : p;
          p = ((mw >> (8 * r)) & 0xffu) ? p : 0.f;
          float dpv = dp[qt][nt][r];
          if constexpr (DROP)
            dpv = drop_keep(md_seed(a.md), a.md.thresh, static_cast<uint32_t>(bh), myq, key) ? dpv * a.md.inv_keep : 0.f;
          s[qt][nt][r] = SOFTCAP ? p * (dpv - dl[qt]) * dcap : p * (dpv - dl[qt]);  // dS^T
        }
      }
    }
    // dQ^T += K^T . dS^T (32 keys per step in the permuted order of the forward's V^T.P^T)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      s8 sb[kQT];
#pragma unroll
      for (int qt = 0; qt < kQT; ++qt) sb[qt] = pack_pair(s[qt][2 * s2], s[qt][2 * s2 + 1]);
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
        const s8 kt = tr_pair(Ks, KP, s2 * 32 + 4 * g, s2 * 32 + 16 + 4 * g, dt * 16, c);
#pragma unroll
        for (int qt = 0; qt < kQT; ++qt) dq[qt][dt] = mfma(kt, sb[qt], dq[qt][dt]);
      }
    }
  }
#pragma unroll
  for (int qt = 0; qt < kQT; ++qt) {
    const int myq = qw + qt * 16 + c;
    if (myq < T) {
      bf16_t* Dp = a.dq + b * a.sdq.b + h * a.sdq.h + static_cast<int64_t>(myq) * a.sdq.t;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
        s4 ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) ov[r] = bfs(dq[qt][dt][r] * a.scale);
        *reinterpret_cast<s4*>(Dp + dt * 16 + 4 * g) = ov;
      }
    }
  }
}

}  // namespace attn
}  // namespace damd

using namespace damd;
using namespace damd::attn;

extern "C" {

// DROP and SOFTCAP never together: the binding refuses softcap > 0 with dropout
// (the head dim / query tiles come last: `64 DAMD_COMMA 1` would split into two arguments here)
#define DAMD_ATTN_DISPATCH_M(KERNEL, MODE_, GRID, ARGS, ...)                                         \
  do {                                                                                               \
    if ((ARGS).md.thresh != 0) DAMD_LAUNCH((KERNEL<__VA_ARGS__, MODE_, true, false>), GRID, dim3(kThreads), 0, st, ARGS); \
    else if ((ARGS).k2 > 0.f) DAMD_LAUNCH((KERNEL<__VA_ARGS__, MODE_, false, true>), GRID, dim3(kThreads), 0, st, ARGS);  \
    else DAMD_LAUNCH((KERNEL<__VA_ARGS__, MODE_, false, false>), GRID, dim3(kThreads), 0, st, ARGS);          \
  } while (0)

#define DAMD_ATTN_DISPATCH_D(KERNEL, D_, GRID, ARGS)                                                \
  do {                                                                                               \
    if ((ARGS).band.klo != nullptr) DAMD_ATTN_DISPATCH_M(KERNEL, kBand, GRID, ARGS, D_);             \
    else if (causal) DAMD_ATTN_DISPATCH_M(KERNEL, kCausal, GRID, ARGS, D_);                          \
    else DAMD_ATTN_DISPATCH_M(KERNEL, kFull, GRID, ARGS, D_);                                        \
  } while (0)

#define DAMD_ATTN_DISPATCH(KERNEL, GRID, ARGS)                                                       \
  do {                                                                                               \
    if (D == 64) DAMD_ATTN_DISPATCH_D(KERNEL, 64, GRID, ARGS);                                       \
    else DAMD_ATTN_DISPATCH_D(KERNEL, 128, GRID, ARGS);                                              \
  } while (0)

// query-tiled kernels (forward, dQ): QT 16-row tiles per wave
#define DAMD_ATTN_DISPATCH_QT(KERNEL, QT, GRID, ARGS)                                                \
  do {                                                                                               \
    if (D == 64) {                                                                                   \
      if ((QT) == 1) DAMD_ATTN_DISPATCH_D(KERNEL, 64 DAMD_COMMA 1, GRID, ARGS);                       \
      else DAMD_ATTN_DISPATCH_D(KERNEL, 64 DAMD_COMMA 2, GRID, ARGS);                                 \
    } else {                                                                                         \
      if ((QT) == 1) DAMD_ATTN_DISPATCH_D(KERNEL, 128 DAMD_COMMA 1, GRID, ARGS);                      \
      else DAMD_ATTN_DISPATCH_D(KERNEL, 128 DAMD_COMMA 2, GRID, ARGS);                                \
    }                                                                                                \
  } while (0)

// Query tiles per wave (measured, B x H x T x D grid of the GPT-2 / BERT shapes, r6 probe):
// the forward prefers QT = 2 (twice the MFMAs per staged K/V tile) except for a small causal
// D = 64 grid, where the heaviest query block is the critical path; the dQ kernel prefers QT = 1
// (half the live accumulators: 4 waves per SIMD at D = 64) up to ~4k workgroups and at D = 128.
// DAMD_ATTN_QT=1|2 forces one (read per launch: the tests switch it).
static int attn_qt(bool dq, int B, int H, int T, int D, int causal) {
  const char* e = getenv("DAMD_ATTN_QT");
  const int forced = e ? atoi(e) : 0;
  if (forced == 1 || forced == 2) return forced;
  const long wgs2 = static_cast<long>(B) * H * ((T + 127) / 128);
  if (dq) return (D == 128 || wgs2 <= 4096) ? 1 : 2;
  return (D == 64 && causal && wgs2 < 2048) ? 1 : 2;
}

static KeyMaskDrop make_md(const uint8_t* km, int64_t kms, uint32_t seed, const int64_t* seedp, float drop_p) {
  KeyMaskDrop md;
  md.km = km;
  md.kms = kms;
  md.seed = seed;
  md.seedp = seedp;
  const double t = static_cast<double>(drop_p) * 4294967296.0;
  md.thresh = drop_p > 0.f ? static_cast<uint32_t>(t >= 4294967295.0 ? 4294967295.0 : (t < 1.0 ? 1.0 : t)) : 0u;
  md.inv_keep = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  return md;
}

// Workgroups per (batch, kv head) group of the grouped-query dK/dV kernel (the head split S).
// The unsplit grid is nblk * B * Hkv workgroups, G times fewer than the MHA kernel's, each with G
// times the work: multi-query attention at a modest batch leaves most of the 256 CUs idle.  Rule:
// double S (up to G) while the grid stays below a target of 1024 workgroups (4 per CU), 2048 from
// T = 4096 on.  Both figures are read off the sweep in profiles/attention_gqa_probe.txt (causal,
// D = 128, H = 32, Hkv in {8, 4, 2, 1}, S in {1 .. G}): at T = 1024 the whole backward is fastest
// with 1024 dK/dV workgroups for every Hkv (Hkv = 1: 1199 us unsplit, 408 at S = 8, 416 at S = 16;
// Hkv = 8: 393 unsplit, 429 at S = 2), at T = 2048 1024 and 2048 workgroups are within 1-2%, and
// at T = 4096 2048 workgroups win by 2-4% for every Hkv (Hkv = 1: 4806 us unsplit, 1331 at S = 8,
// 1285 at S = 16, 1325 at S = 32).  Lengths between 2048 and 4096 and D = 64 were not swept.
// DAMD_ATTN_GQA_SPLIT=<S> forces it (clamped to [1, G]; read per launch: the tests switch it).
int damd_attn_gqa_split(int B, int Hkv, int G, int T) {
  const char* e = getenv("DAMD_ATTN_GQA_SPLIT");
  const int forced = e ? atoi(e) : 0;
  if (forced >= 1) return forced < G ? forced : G;
  const long wgs = static_cast<long>(B) * Hkv * ((T + kBlk - 1) / kBlk), target = T >= 4096 ? 2048 : 1024;
  int S = 1;
  while (2 * S <= G && wgs * S < target) S *= 2;
  return S;
}

// delta = rowsum(dO . O) for the D = 256 backward (attention_d256.hip); so / sdo: (b, h, t) strides.
void damd_attn_delta256_launch(const void* o, const int64_t* so, const void* dout, const int64_t* sdo, float* delta,
                               int B, int H, int T, hipStream_t st) {
  const int64_t rows = static_cast<int64_t>(B) * H * T;
  const int blocks = static_cast<int>((rows * 32 + 255) / 256);
  const Strides os{so[0], so[1], so[2]}, ds{sdo[0], sdo[1], sdo[2]};
  DAMD_LAUNCH((attn_delta_kernel<256>), dim3(blocks), dim3(256), 0, st, static_cast<const bf16_t*>(o), os,
              static_cast<const bf16_t*>(dout), ds, delta, H, T, rows);
}

// strides: 4 tensors (q, k, v, o) x (b, h, t) in elements; km: optional [B][kms] key mask.
// softcap: the logit cap c (0: none; >= 0, finite and without dropout: checked by the binding), scores
// become c * tanh(q.k * scale / c) before the masks.
// klo .. qhi: the band arrays (all four or none; with them `causal` only feeds attn_qt), rows of
// band_stride int32 (0: one shared row), padded to a multiple of 128 entries >= T.
// k, v have Hkv heads, H % Hkv == 0 (checked by the binding).
void damd_attn_fwd_launch(const void* q, const void* k, const void* v, void* o, float* lse, const int64_t* strides,
                          int B, int H, int Hkv, int T, int D, float scale, int causal, const uint8_t* km,
                          int64_t kms, uint32_t seed, const int64_t* seedp, float drop_p, hipStream_t st,
                          const int32_t* klo, const int32_t* khi, const int32_t* qlo, const int32_t* qhi,
                          int64_t band_stride, float softcap) {
  FwdArgs a;
  a.k1 = cap_k1(scale, softcap); a.k2 = softcap * kLog2e;
  a.q = static_cast<const bf16_t*>(q); a.k = static_cast<const bf16_t*>(k); a.v = static_cast<const bf16_t*>(v);
  a.o = static_cast<bf16_t*>(o); a.lse = lse;
  a.sq = {strides[0], strides[1], strides[2]}; a.sk = {strides[3], strides[4], strides[5]};
  a.sv = {strides[6], strides[7], strides[8]}; a.so = {strides[9], strides[10], strides[11]};
  a.H = H; a.T = T; a.G = H / Hkv; a.scale_log2 = scale * kLog2e;
  a.md = make_md(km, kms, seed, seedp, drop_p);
  a.band = {klo, khi, qlo, qhi, band_stride};
  const int qt = attn_qt(false, B, H, T, D, causal), rows = fwd_rows(qt);
  dim3 grid(((T + rows - 1) / rows) * H * B);
  DAMD_ATTN_DISPATCH_QT(attn_fwd_kernel, qt, grid, a);
}

// strides: 8 tensors (q, k, v, o, dout, dk, dv, dq) x (b, h, t).  k, v, dk, dv have Hkv heads.
// Hkv < H: `split` is damd_attn_gqa_split(...) as the caller read it, and for split > 1 `part` holds
// 2 * split * B * Hkv * T * D floats.
void damd_attn_bwd_launch(const void* q, const void* k, const void* v, const void* o, const void* dout,
                          const float* lse, float* delta, float* part, int split, void* dq, void* dk, void* dv,
                          const int64_t* s, int B, int H, int Hkv, int T, int D, float scale, int causal,
                          const uint8_t* km, int64_t kms, uint32_t seed, const int64_t* seedp, float drop_p,
                          hipStream_t st, const int32_t* klo, const int32_t* khi, const int32_t* qlo,
                          const int32_t* qhi, int64_t band_stride, float softcap) {
  const Strides sq{s[0], s[1], s[2]}, sk{s[3], s[4], s[5]}, sv{s[6], s[7], s[8]}, so{s[9], s[10], s[11]},
      sdo{s[12], s[13], s[14]}, sdk{s[15], s[16], s[17]}, sdv{s[18], s[19], s[20]}, sdq{s[21], s[22], s[23]};
  const int64_t rows = static_cast<int64_t>(B) * H * T;
  {
    const int64_t threads = rows * (D / 8);
    const int blocks = static_cast<int>((threads + 255) / 256);
    if (D == 64)
      DAMD_LAUNCH((attn_delta_kernel<64>), dim3(blocks), dim3(256), 0, st, static_cast<const bf16_t*>(o), so,
                         static_cast<const bf16_t*>(dout), sdo, delta, H, T, rows);
    else
      DAMD_LAUNCH((attn_delta_kernel<128>), dim3(blocks), dim3(256), 0, st, static_cast<const bf16_t*>(o),
                         so, static_cast<const bf16_t*>(dout), sdo, delta, H, T, rows);
    DAMD_CHECK_LAUNCH();
  }
  BwdArgs a;
  a.q = static_cast<const bf16_t*>(q); a.k = static_cast<const bf16_t*>(k); a.v = static_cast<const bf16_t*>(v);
  a.dout = static_cast<const bf16_t*>(dout); a.lse = lse; a.delta = delta; a.dq_acc = nullptr;
  a.dk = static_cast<bf16_t*>(dk); a.dv = static_cast<bf16_t*>(dv);
  a.sq = sq; a.sk = sk; a.sv = sv; a.sdo = sdo; a.sdk = sdk; a.sdv = sdv;
  a.H = H; a.T = T; a.scale = scale; a.scale_log2 = scale * kLog2e;
  a.G = H / Hkv; a.S = a.G > 1 ? split : 1; a.part = part;
  a.md = make_md(km, kms, seed, seedp, drop_p);
  a.band = {klo, khi, qlo, qhi, band_stride};
  a.k1 = cap_k1(scale, softcap); a.k2 = softcap * kLog2e;
  const int nblk = (T + kBlk - 1) / kBlk;
  if (a.G == 1) {
    dim3 grid(nblk * H * B);
    DAMD_ATTN_DISPATCH(attn_bwd_kernel, grid, a);
  } else {
    dim3 grid(nblk * Hkv * B * a.S);
    DAMD_ATTN_DISPATCH(attn_bwd_gqa_kernel, grid, a);
    if (a.S > 1) {
      const int64_t plane = static_cast<int64_t>(B) * Hkv * T * D;
      DAMD_LAUNCH(attn_gqa_sum_kernel, dim3(static_cast<unsigned>((plane / 4 + 255) / 256)), dim3(256), 0, st, part,
                  a.S, a.dk, sdk, a.dv, sdv, Hkv, T, D, plane);
      DAMD_CHECK_LAUNCH();
    }
  }
  DqArgs d;
  d.q = a.q; d.k = a.k; d.v = a.v; d.dout = a.dout; d.lse = lse; d.delta = delta;
  d.dq = static_cast<bf16_t*>(dq);
  d.sq = sq; d.sk = sk; d.sv = sv; d.sdo = sdo; d.sdq = sdq;
  d.H = H; d.T = T; d.G = a.G; d.scale = scale; d.scale_log2 = scale * kLog2e;
  d.md = a.md;
  d.band = a.band;
  d.k1 = a.k1; d.k2 = a.k2;
  const int qt = attn_qt(true, B, H, T, D, causal), qrows = fwd_rows(qt);
  dim3 qgrid(((T + qrows - 1) / qrows) * H * B);
  DAMD_ATTN_DISPATCH_QT(attn_dq_kernel, qt, qgrid, d);
}

}  // extern "C"
