// Chunked-prefill attention for gfx950 / MI355X: a query chunk of tens to thousands of rows at the
// END of a longer key / value sequence (the second turn of a chat against a kept cache, chunked
// prefill, long draft chunks).  bf16 in/out, fp32 accumulate, forward only.
//   q [B, H, Tq, D], k / v [B, Hkv, Tk, D], H % Hkv == 0, 1 <= Tq <= Tk, D in {64, 128};
//   query row i sits at absolute position p = Tk - Tq + i (bottom-right alignment);
//   causal: key j <= p; window W (with causal): also j >= p - W + 1; optional uint8 key mask --
//   the masks of attention_decode.hip, which keeps the calls with (H / Hkv) * Tq <= 32 packed rows.
//
// Neither sibling fits the shape: the forward (attention.hip) has one T and one workgroup per (query
// block, head), so a 64-row chunk is a handful of workgroups that each walk every key tile and every
// head of a group stages the same K/V again; the decoder gives each WAVE private K/V tiles, which is
// right for <= 32 rows and wasteful for hundreds.  This kernel is query-major with K/V staged once
// per workgroup (the forward's tile body) and has the decoder's alignment, group packing and key
// split.
//
// Packed rows, position-major.  The R = G * Tq query rows of one (batch, K/V head), G = H / Hkv, are
//   ordered rr = i * G + hg: a workgroup's 64 * QT rows are ALL G heads of 64 * QT / G consecutive
//   positions (G need not divide it, nor be a power of two).  The rows of a block then differ in
//   position by at most 64 * QT / G, so their causal / window bounds nearly coincide and at most two
//   tiles per edge are masked, and every staged K/V tile serves the whole group: one HBM / L2 read
//   per K/V head, not G.  Each lane carries its row's (head, position): the Q fragments are loaded
//   once through the row's own (h, t) strides and stay in registers, and the mask is two integer
//   compares against the lane's [kmin, kmax].
// Tile body (the forward's).  S^T = K.Q^T with the query on the lane, lane-local online softmax,
//   O^T = V^T.P^T straight from the S^T accumulators with V read by ds_read_b64_tr_b16.  The 64-key
//   K and V tiles are staged in LDS once per workgroup and used by its four waves; the next tile's
//   global loads are issued into registers before the current tile's MFMAs.  QT in {1, 2} 16-row
//   tiles per wave.  Interior tiles -- every key < Tk, <= the block's first position and >= its
//   last position - W + 1, no key mask -- run a body compiled without masking between masked edge
//   tiles.  Unlike the forward this holds at D = 128 too: there the three loop copies cost no
//   occupancy (one masked body: 154 VGPRs / 3 waves at QT = 1, 240 / 2 at QT = 2; with the copies the
//   table below), so the kernel has one loop structure for both head sizes.
// Tile range and key split.  Grid (query blocks, S, B * Hkv).  A block visits the tiles from the one
//   holding the lowest key in the window of its first position to the one holding its last position
//   (causal) or the last key (full); split s owns a contiguous share of THAT range, so the splits of
//   a block are even whatever the block's causal end.  A split without a tile is legal and
//   contributes m = -inf, l = 0, O = 0.  Under a causal mask the blocks are dispatched last (longest)
//   first.
// Epilogue.  S == 1 writes bf16 o ([B, Tq, H, D] memory) and the log-sum-exp.  S > 1 writes fp32
//   partials O [S, B, H, Tq, D] (unnormalised) and (m, l) [2, S, B, H, Tq], the layout and convention
//   of attention_decode.hip, whose attn_decode_combine_kernel finishes the call.  A row with no
//   attendable key gives zeros and lse = -inf.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no instantiation spills):
//   attn_chunk_kernel<D, QT>     VGPRs (+AGPRs)  SGPRs  LDS bytes  waves / SIMD  scratch
//     <64, 1>                    108             74     20480      4             0
//     <64, 2>                    164             74     20480      3             0
//     <128, 1>                   152             76     36864      3             0
//     <128, 2>                   247             85     36864      2             0
//   (attn_decode_combine_kernel: attention_decode.hip)
#include "common.h"
#include "attention_frag.h"

#include <math.h>

#include <stdlib.h>

#include <type_traits>

namespace damd {
namespace attn {

struct ChunkArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o; float* lse;
  float* po; float* pml;  // S > 1: fp32 partials O [S][B][H][Tq][D], (m, l) [2][S][B][H][Tq]
  Strides sq, sk, sv, so;
  int B, H, G, Tq, Tk;
  int S;               // key split (gridDim.y)
  int causal, window;  // window 0: none
  float scale_log2;    // softmax scale * log2(e)
  const uint8_t* km;   // [B][kms] key validity (nullptr: every key < Tk is valid)
  int64_t kms;
};

// A 64-key x D bf16 tile through the workgroup's 256 threads: global -> registers (issued a tile
// ahead), registers -> the row-major LDS image (row stride kLdsStride(D)).  Keys >= Tk are zeros
// (their probabilities are zero; the data must not be NaN).  The forward's staging (attention.hip
// Stage<D, 64>), which lives in that translation unit.
template <int D>
struct KVStage {
  static constexpr int CH = D / 8, N = kBlk * CH / kThreads;
  s8 r[N];
  __device__ __forceinline__ void load(const bf16_t* __restrict__ base, int64_t st, int k0, int Tk) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int idx = threadIdx.x + i * kThreads, row = idx / CH, col = (idx % CH) * 8;
      s8 x = {0, 0, 0, 0, 0, 0, 0, 0};
      if (k0 + row < Tk) x = *reinterpret_cast<const s8*>(base + static_cast<int64_t>(k0 + row) * st + col);
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

template <int D, int QT>
__global__ void __launch_bounds__(kThreads) attn_chunk_kernel(ChunkArgs a) {
  constexpr int KP = kLdsStride(D), ROWS = 64 * QT;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[kBlk * KP];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[kBlk * KP];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
  const int s = blockIdx.y, bkv = blockIdx.z, Hkv = a.H / a.G, hkv = bkv % Hkv, b = bkv / Hkv;
  const int Tk = a.Tk, Tq = a.Tq, G = a.G, R = G * Tq, base = Tk - Tq;
  const int qb = a.causal ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const int rr0 = qb * ROWS, rw = rr0 + w * 16 * QT;  // first packed row of the block / of this wave
  const bf16_t* Kp = a.k + b * a.sk.b + hkv * a.sk.h;
  const bf16_t* Vp = a.v + b * a.sv.b + hkv * a.sv.h;
  const uint8_t* KMp = a.km ? a.km + b * a.kms : nullptr;

  // the block's positions [p_first, p_last] and its tiles: visited [tb, te), this split's [t0, t1),
  // and [full_lo, full_hi) inside every valid row's key range
  const int p_first = base + rr0 / G, p_last = base + (min(rr0 + ROWS, R) - 1) / G;
  const int lo_first = a.window > 0 ? max(p_first - a.window + 1, 0) : 0;
  const int lo_last = a.window > 0 ? max(p_last - a.window + 1, 0) : 0;
  const int tb = lo_first / kBlk, te = a.causal ? p_last / kBlk + 1 : (Tk + kBlk - 1) / kBlk;
  const int t0 = tb + static_cast<int>(static_cast<int64_t>(s) * (te - tb) / a.S);
  const int t1 = tb + static_cast<int>(static_cast<int64_t>(s + 1) * (te - tb) / a.S);
  const int full_lo = (lo_last + kBlk - 1) / kBlk;
  const int full_hi = a.causal ? min((p_first + 1) / kBlk, Tk / kBlk) : Tk / kBlk;

  // the lane's packed row per 16-row tile: Q fragments and the key range [kmin, kmax] of its position
  s8 qf[QT][D / 32];
  int kmin[QT], kmax[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int rr = rw + qt * 16 + c, i = rr / G, hg = rr - i * G, pos = base + i;
    const bool valid = rr < R;
    kmax[qt] = valid ? (a.causal ? pos : Tk - 1) : -1;  // a row past R attends nothing and is never written
    kmin[qt] = a.window > 0 ? pos - a.window + 1 : 0;
    const bf16_t* Qp = a.q + b * a.sq.b + (hkv * G + hg) * a.sq.h + static_cast<int64_t>(i) * a.sq.t;
#pragma unroll
    for (int ds = 0; ds < D / 32; ++ds) {
      s8 x = {0, 0, 0, 0, 0, 0, 0, 0};
      if (valid) x = *reinterpret_cast<const s8*>(Qp + ds * 32 + 8 * g);
      qf[qt][ds] = x;
    }
  }
  f4 oacc[QT][D / 16];
  float m[QT], l[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    m[qt] = -INFINITY;
    l[qt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) oacc[qt][dt] = f4{0.f, 0.f, 0.f, 0.f};
  }

  KVStage<D> ks, vs;
  if (t0 < t1) {
    ks.load(Kp, a.sk.t, t0 * kBlk, Tk);
    vs.load(Vp, a.sv.t, t0 * kBlk, Tk);
  }
  auto tile = [&](int t, auto masked) {
    constexpr bool MASK = decltype(masked)::value;
    const int k0 = t * kBlk;
    __syncthreads();  // every wave has read the previous tile
    ks.store(Ks);
    vs.store(Vs);
    __syncthreads();
    if (t + 1 < t1) {  // next tile's loads fly under this tile's MFMAs
      ks.load(Kp, a.sk.t, k0 + kBlk, Tk);
      vs.load(Vp, a.sv.t, k0 + kBlk, Tk);
    }
    f4 sc[QT][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) sc[qt][nt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < D / 32; ++ds) {
        const s8 kf = *reinterpret_cast<const s8*>(Ks + (nt * 16 + c) * KP + ds * 32 + 8 * g);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) sc[qt][nt] = mfma(kf, qf[qt][ds], sc[qt][nt]);
      }
    }
    // per-key validity of the lane's 16 keys (mask rows are padded to a multiple of 64 keys: the
    // word loads stay inside the row)
    uint32_t mw[4];
    if constexpr (MASK) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        mw[nt] = KMp ? *reinterpret_cast<const uint32_t*>(KMp + k0 + nt * 16 + 4 * g) : 0x01010101u;
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      // raw scores; the softmax scale (> 0) is folded into the exp2 argument: p = 2^(s*c - m)
      float mx = -INFINITY;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (MASK) {
            const int key = k0 + nt * 16 + 4 * g + r;
            const bool out = key > kmax[qt] || key < kmin[qt] || ((mw[nt] >> (8 * r)) & 0xffu) == 0;
            sc[qt][nt][r] = out ? -INFINITY : sc[qt][nt][r];
          }
          mx = fmaxf(mx, sc[qt][nt][r]);
        }
      mx = rows_max(mx);
      const float m_new = fmaxf(m[qt], mx * a.scale_log2);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = ex2(m[qt] - m_use);
      float rs = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = ex2(fmaf(sc[qt][nt][r], a.scale_log2, -m_use));
          rs += p;
          sc[qt][nt][r] = p;
        }
      l[qt] = l[qt] * alpha + rs;
      m[qt] = m_new;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) oacc[qt][dt] *= alpha;
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      s8 pb[QT];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) pb[qt] = pack_pair(sc[qt][2 * s2], sc[qt][2 * s2 + 1]);
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
        const s8 vf = tr_pair(Vs, KP, s2 * 32 + 4 * g, s2 * 32 + 16 + 4 * g, dt * 16, c);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) oacc[qt][dt] = mfma(vf, pb[qt], oacc[qt][dt]);
      }
    }
  };
  int t = t0;
  if (!KMp) {
    for (const int e = min(full_lo, t1); t < e; ++t) tile(t, std::true_type{});
    for (const int e = min(full_hi, t1); t < e; ++t) tile(t, std::false_type{});
  }
  for (; t < t1; ++t) tile(t, std::true_type{});

  const int64_t rows = static_cast<int64_t>(a.B) * a.H * Tq;
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float lt = rows_sum(l[qt]);
    const int rr = rw + qt * 16 + c, i = rr / G, h = hkv * G + rr - i * G;
    if (rr >= R) continue;
    const int64_t row = (static_cast<int64_t>(b) * a.H + h) * Tq + i;
    if (a.S == 1) {
      const float inv = lt > 0.f ? 1.f / lt : 0.f;
      bf16_t* Op = a.o + b * a.so.b + h * a.so.h + static_cast<int64_t>(i) * a.so.t;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
        s4 ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) ov[r] = bfs(oacc[qt][dt][r] * inv);
        *reinterpret_cast<s4*>(Op + dt * 16 + 4 * g) = ov;
      }
      if (g == 0) a.lse[row] = lt > 0.f ? m[qt] * kLn2 + logf(lt) : -INFINITY;
    } else {
      float* Pp = a.po + (s * rows + row) * D;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) *reinterpret_cast<f4*>(Pp + dt * 16 + 4 * g) = oacc[qt][dt];
      if (g == 0) {
        a.pml[s * rows + row] = m[qt];
        a.pml[(a.S + s) * rows + row] = lt;
      }
    }
  }
}

}  // namespace attn
}  // namespace damd

using namespace damd;
using namespace damd::attn;

extern "C" {

// attention_decode.hip: o / lse from the fp32 partials of `split` key splits
void damd_attn_decode_combine_launch(const float* po, const float* pml, int split, void* o, const int64_t* so,
                                     float* lse, int B, int H, int Tq, int D, hipStream_t st);

// The key split S (returned) and the query tiles per wave QT of a call.  The decode launcher's rule
// divided by the number of query blocks: S grows until the grid (query blocks x S x B * Hkv) reaches
// QT workgroups per CU while a split of the longest block keeps at least 8 tiles; QT = 2 (twice the
// MFMAs per staged tile, half the blocks) once the QT = 2 grid has a workgroup for every other CU
// before any split.  Read off the forced (QT, S) sweep in profiles/attention_chunk_probe.txt (causal,
// call time, S in {1, 2, 4, 8, 16}); the rule lands on the sweep's minimum or within 2% of it for
// every shape there.  B1 H32 Hkv8 D128 Tk 8192: Tq 16 (one block) 149 us unsplit, 25 at QT 1 S 16;
// Tq 64 fastest at QT 1 S 8 (32 us; S 16 36, QT 2 S 16 36); Tq 512 at QT 2 S 4 (102 us; QT 1 at best
// 119); Tq 2048 at QT 2 unsplit (327 us; QT 1 382).  B8 of the same at Tq 64: QT 2 S 4 (117 us; QT 1 at
// best 156).  MHA B4 H16 D64 Tq 128 Tk 2048: QT 1 S 2 .. 4 (20 us; QT 2 21).  Past the target the fp32
// partials (S x B x H x Tq x D) cost more than the parallelism gives: Tq 2048 loses 53% from S 1 to 16.
// DAMD_ATTN_DECODE_SPLIT=<S> forces S (clamped to [1, 256], not to the tile count: splits without a
// tile are legal) and DAMD_ATTN_QT=1|2 forces QT, both read per launch: the tests and the probe
// switch them.
int damd_attn_chunk_plan(int B, int Hkv, int G, int Tq, int Tk, int D, int window, int* qt_out) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    DAMD_CHECK(hipGetDevice(&dev));
    DAMD_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    cus = n > 0 ? n : 256;
  }
  const int64_t R = static_cast<int64_t>(G) * Tq, units = static_cast<int64_t>(B) * Hkv;
  const char* eq = getenv("DAMD_ATTN_QT");
  const int fqt = eq ? atoi(eq) : 0;
  const int qt = fqt == 1 || fqt == 2 ? fqt : (2 * units * ((R + 127) / 128) >= cus ? 2 : 1);
  *qt_out = qt;
  const char* es = getenv("DAMD_ATTN_DECODE_SPLIT");
  const int forced = es ? atoi(es) : 0;
  if (forced >= 1) return forced < 256 ? forced : 256;
  // the tiles of the last (longest) query block
  const int64_t nqb = (R + 64 * qt - 1) / (64 * qt);
  const int p_first = Tk - Tq + static_cast<int>((nqb - 1) * 64 * qt / G);
  const int lo = window > 0 && p_first - window + 1 > 0 ? p_first - window + 1 : 0;
  const int64_t tiles = (Tk + kBlk - 1) / kBlk - lo / kBlk, cap = tiles / 8;
  int64_t S = (int64_t{qt} * cus + units * nqb - 1) / (units * nqb);
  if (S > cap) S = cap;
  if (S > 256) S = 256;
  return S < 1 ? 1 : static_cast<int>(S);
}

// strides: 4 tensors (q, k, v, o) x (b, h, t) in elements; km: optional [B][kms] key mask with
// kms >= pad64(Tk).  k, v have Hkv heads, H % Hkv == 0, 1 <= Tq <= Tk, (H / Hkv) * Tq < 2^31 - 128
// (checked by the binding).  split and qt: damd_attn_chunk_plan(...) as the caller read it; split > 1:
// po holds split * B * H * Tq * D floats, pml 2 * split * B * H * Tq.
void damd_attn_chunk_launch(const void* q, const void* k, const void* v, void* o, float* lse, float* po, float* pml,
                            const int64_t* strides, int B, int H, int Hkv, int Tq, int Tk, int D, float scale,
                            int causal, int window, const uint8_t* km, int64_t kms, int split, int qt,
                            hipStream_t st) {
  ChunkArgs a;
  a.q = static_cast<const bf16_t*>(q); a.k = static_cast<const bf16_t*>(k); a.v = static_cast<const bf16_t*>(v);
  a.o = static_cast<bf16_t*>(o); a.lse = lse; a.po = po; a.pml = pml;
  a.sq = {strides[0], strides[1], strides[2]}; a.sk = {strides[3], strides[4], strides[5]};
  a.sv = {strides[6], strides[7], strides[8]}; a.so = {strides[9], strides[10], strides[11]};
  a.B = B; a.H = H; a.G = H / Hkv; a.Tq = Tq; a.Tk = Tk;
  a.S = split;
  a.causal = causal; a.window = window; a.scale_log2 = scale * kLog2e;
  a.km = km; a.kms = kms;
  const int64_t R = static_cast<int64_t>(a.G) * Tq;
  const dim3 grid(static_cast<unsigned>((R + 64 * qt - 1) / (64 * qt)), split, B * Hkv);
  if (D == 64) {
    if (qt == 2) DAMD_LAUNCH((attn_chunk_kernel<64, 2>), grid, dim3(kThreads), 0, st, a);
    else DAMD_LAUNCH((attn_chunk_kernel<64, 1>), grid, dim3(kThreads), 0, st, a);
  } else {
    if (qt == 2) DAMD_LAUNCH((attn_chunk_kernel<128, 2>), grid, dim3(kThreads), 0, st, a);
    else DAMD_LAUNCH((attn_chunk_kernel<128, 1>), grid, dim3(kThreads), 0, st, a);
  }
  if (split > 1) damd_attn_decode_combine_launch(po, pml, split, o, strides + 9, lse, B, H, Tq, D, st);
}

}  // extern "C"
