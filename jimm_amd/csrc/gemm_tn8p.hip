// K15 — TN weight-gradient GEMM: dW[N,Kw] = dz^T @ X (contraction over the
// huge M = B*L dimension), 256x256 output tiles, split-M, MFMA bf16.
//
// Both operands are stored m-major ([M,N] / [M,Kw]) so both MFMA fragments
// need per-lane m-columns.  Staging: global_load_lds (glds, 16 B per lane)
// straight into a transpose-friendly LDS image, with the image permutation
// on the per-lane SOURCE address (glds writes lane-linear); fragments come
// back by ds_read_b64_tr_b16 (the gfx950 hardware transpose read — no
// builtin, inline asm per guide §5.7 form (i): reads + their s_waitcnt
// lgkmcnt(0) in ONE statement, outputs "=&v").
//
// Unit image (16 KiB per operand, one 32-m x 256-col K-half):
//   byte(m, col) = nt*1024 + qpos*128 + jm*32 + u*16
//   with q' = (m>>2)&7, jm = m&3, qpos = (q'&1)*4+(q'>>1) (even m-quads
//   first, then odd), nt = col>>4, u = (col>>3)&1.
// A ds_read_b64_tr_b16 at per-lane address base + lane*8 delivers lane
// (lo,hi) the 4 elements m = 8*hi + (0..3) of column nt*16 + lo (the odd
// quads via immediate offset +512) — exactly the MFMA fragment m-octet per
// hi group, with the 32-lane groups touching disjoint bank rows (the
// verified T10 subtile pattern).
//
// Staging ring.  The unit of staging is one K-half u = 2*tile + kh of a
// full 64-row tile: 2 glds per thread for dz + 2 for X, landing in one
// 32 KiB slot (dz image at +0, X image at +16 KiB).  LDS is a ring of
// RING = 5 slots (160 KiB, the full CU LDS, as the forward kernel; measured
// 1-3% over a 4-slot ring); unit u lives in slot u % RING.  Each unit is
// consumed in two phases (pr = n-half of the output tile), one raw
// s_barrier per phase, X-side fragments reused in registers across the pr
// pair:
//   A(u): tr-read X frags + dz frags (pr0) of slot(u); lgkmcnt(0);
//         barrier BA(u); 16 MFMA
//   B(u): tr-read dz frags (pr1); lgkmcnt(0); counted vmcnt; barrier
//         BB(u); issue unit u+RING into slot(u); 16 MFMA
// (Issuing a phase's reads one phase ahead, under the wave's own MFMAs,
// measured 1-4% slower on every ViT-B shape and was not kept;
// profiles/dw_readahead_NOTES.md section 4.)
// Certification:
//   RAW  unit v is first read in A(v), after barrier BB(v-1).  Before
//        arriving at BB(v-1) every wave waits until its own pieces of v
//        have landed: it has issued units up to v+RING-2 by then and vmcnt
//        retires loads in order, so s_waitcnt vmcnt(4*(RING-2)) (4 glds per
//        unit; fewer newer units near the end of the stream: 4*(units
//        still behind v), 0 only for the last unit) covers v.  BB(v-1) then
//        makes all waves' pieces visible.  The prologue issues units
//        0..RING-1, waits down to unit 0 the same way and raises one
//        barrier before A(0).
//   WAR  slot(u) is rewritten by unit u+RING, issued after BB(u).  Every
//        wave's last reads of unit u are in B(u) and are retired by the
//        lgkmcnt(0) of that asm block, i.e. before the wave arrives at
//        BB(u); a glds issued after BB(u) cannot overtake them.
//   So RING-1 units (2 tiles) are in flight across barriers and no wave
//   drains the queue inside the loop.  The counted wait is exact because
//   the loop holds no other vector-memory instruction.
// Ragged tail: a last tile with fewer than 64 rows cannot go by glds (no
// zero fill).  It is staged after the ring has drained (the last unit's
// wait is vmcnt(0) and BB(last) has passed, so every slot is free):
// guarded coalesced register loads, scattered ds_write_b128 into slots
// 0/1, one barrier, then the same two-phase walk.  M-tail rows load zeros
// (no clamping — this is an accumulation).
//
// Bias fold (DBOUT): db[n] = sum_m dz[m][n] comes out of the dz fragments
// already in registers.  The four waves of equal wm hold the same dz
// fragments and the nt_k workgroups of one (n-tile, split) see the same dz,
// so the work is dealt out: wave (wm, wn) folds fragment mi = wn only, and
// of the chunk's 32-row units (ring units, then the tail's two) workgroup
// k-tile kt folds those with unit % P == kt, P = min(nt_k, FOLD_PMAX);
// k-tiles >= P fold nothing.  Each unit of each chunk is counted once; at
// the end a folding wave adds its 2 x 16 columns with one atomic each.
//
// Split-M: grid.y walks m-chunks (slow index -> the chunk's operand rows
// stay L3-resident across its output tiles).  Each split writes a private
// fp32 slice of a workspace and ws_reduce_kernel folds them in fixed order
// (deterministic), writing fp32 or bf16; grid.y == 1 stores once, straight
// into C.
//
// RAGGED (gemm_tn_8p_ragged): any N % 8 == 0, Kw % 8 == 0 on
// ceil(N/256) x ceil(Kw/256) tiles, for weight shapes off the 256 grid with
// too many 128-tiles for gemm_tn128.hip (so400m's 4304 x 1152).  The loop, the
// ring, the barriers and the counted waits are the ones above; the flag adds
// no vector-memory instruction to the loop.  N and Kw are OUTPUT dimensions,
// so an edge needs no zero fill:
//   staging  a lane whose 8-column chunk starts at or beyond N (Kw) reads the
//            chunk at N - 8 (Kw - 8) of the same row instead — valid and
//            16-byte aligned — in the ring (the clamp is on the source
//            pointers, made once) and in the register-staged tail (which
//            keeps its zero rows).  What it brings in lands only in
//            accumulator rows >= N / columns >= Kw.
//   skipping a wave's 64 x 64 sub-block of row half pr that starts at or
//            beyond N or Kw has no tr-reads and no MFMAs in phase pr; the
//            wave still stages, waits and arrives at both barriers.  (WAR
//            holds: a wave without reads has none to retire.)
//   stores   the direct and the workspace store are predicated on n < N,
//            k < Kw; the workspace is [split][N][Kw], so tn_ws_reduce applies
//            unchanged and dW stays bitwise deterministic.
//   fold     dealt out as above with P from the ragged k-tile count, atomics
//            predicated on n < N.  A wave skipped for its k-columns alone
//            still folds: it reads the one dz fragment it owns (mi = wn).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <climits>

#include "mfma.h"

namespace {

typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef short bf16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int BN = 256, BKW = 256, BMS = 64;  // n-tile, k-tile, m-step
constexpr int NTHREADS = 512;
constexpr int BMU = 32;             // m-rows per staging unit (one K-half)
constexpr int UNIT_BYTES = 16384;   // one operand's 32x256 bf16 unit image
constexpr int SLOT_BYTES = 2 * UNIT_BYTES;  // dz image + X image
constexpr int RING = 5;             // ring slots (RING * 32 KiB of LDS)
constexpr int GLDS_PER_UNIT = 4;    // per thread: 2 dz + 2 X
constexpr int FOLD_PMAX = 4;        // k-tiles of one n-tile that share the bias fold

// Counted wait: returns once at most the `newer` most recently issued
// units of this wave are still in flight (vmcnt retires glds in order).
__device__ __forceinline__ void wait_units_in_flight(int newer) {
  static_assert(GLDS_PER_UNIT == 4 && RING == 5, "vmcnt literals below");
  switch (newer) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
  }
}

// unit-image byte offset of element (m_local 0..31, col 0..255)
__device__ __forceinline__ int img_off(int m, int col) {
  const int q = (m >> 2) & 7, jm = m & 3;
  const int qpos = (q & 1) * 4 + (q >> 1);
  return (col >> 4) * 1024 + qpos * 128 + jm * 32 + ((col >> 3) & 1) * 16;
}

// inverse: unit-image byte offset o (16-B granular) -> (m_local, col)
__device__ __forceinline__ void img_inv(int o, int& m, int& col) {
  const int nt = (o >> 10) & 15;
  const int qpos = (o >> 7) & 7;
  const int jm = (o >> 5) & 3;
  const int u = (o >> 4) & 1;
  const int q = ((qpos >> 2) & 1) + (qpos & 3) * 2;
  m = q * 4 + jm;
  col = nt * 16 + u * 8;
}

template <bool DBOUT, bool WSOUT, bool RAGGED = false>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_tn_8p_kernel(
    const bf16* __restrict__ DZ, const bf16* __restrict__ X, float* __restrict__ C,
    int64_t M, int N, int Kw, int64_t chunk_m, float* __restrict__ DB) {
  // ring slot s at s*32 KiB: dz unit image at +0, X unit image at +16 KiB
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wave = tid / WAVE;
  const int lo = lane & 15, hi = lane >> 4;

  const int nt_n = RAGGED ? (N + BN - 1) / BN : N / BN;
  const int nt_k = RAGGED ? (Kw + BKW - 1) / BKW : Kw / BKW;
  const int wg = xcd_remap(blockIdx.x, nt_n * nt_k);
  const int n0 = (wg / nt_k) * BN;
  const int k0 = (wg % nt_k) * BKW;
  const int wm = wave >> 2;  // 0..1 (n sub-position)
  const int wn = wave & 3;   // 0..3 (k sub-position)

  const int64_t m_begin = (int64_t)blockIdx.y * chunk_m;
  const int64_t m_end = m_begin + chunk_m < M ? m_begin + chunk_m : M;
  if (m_end <= m_begin) return;
  const int nfull = (int)((m_end - m_begin) / BMS);  // full 64-row tiles
  const int nunit = 2 * nfull;                       // ring units
  const bool tail = (m_end - m_begin) % BMS != 0;

  // RAGGED: live[pr] — this wave's 64 x 64 output sub-block of row half pr
  // reaches into the matrix (wave-uniform, in scalar registers); a dead
  // sub-block has no tr-reads and no MFMAs (header).
  bool live[2] = {true, true};
  if constexpr (RAGGED) {
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const bool live_k = k0 + (wv & 3) * 64 < Kw;
    live[0] = live_k && n0 + (wv >> 2) * 64 < N;
    live[1] = live_k && n0 + 128 + (wv >> 2) * 64 < N;
  }

  f32x4_t acc[2][4][4] = {};  // [pr][mi][ni]
  // DBOUT: db[n] = sum_m dz[m][n] folded out of the A fragments already in
  // registers (the separate colsum kernel re-reads dz from HBM), dealt out
  // over waves and k-tiles (header): this wave folds fragment mi = wn of the
  // units fold_at, fold_at + fold_p, ...; k-tiles >= fold_p never fold.
  float db_acc[2] = {};
  const int wn_u = __builtin_amdgcn_readfirstlane(wn);  // scalar, for the switch
  const int kt = wg % nt_k;
  const int fold_p = nt_k < FOLD_PMAX ? nt_k : FOLD_PMAX;
  int fold_at = kt < fold_p ? kt : INT_MAX;  // next unit of the chunk to fold
  int unit_no = 0;                           // ring units, then the tail's two
  // sum of one fragment's 8 dz values (this lane's column, 8 rows)
  auto sum8 = [](const bf16x8_t& a) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += __uint_as_float((unsigned int)(unsigned short)a[j] << 16);
    return s;
  };
  auto fold = [&](const bf16x8_t (&ad)[4], int pr) __attribute__((always_inline)) {
    switch (wn_u) {
      case 0: db_acc[pr] += sum8(ad[0]); break;
      case 1: db_acc[pr] += sum8(ad[1]); break;
      case 2: db_acc[pr] += sum8(ad[2]); break;
      default: db_acc[pr] += sum8(ad[3]); break;
    }
  };

  // Ring staging for this thread: glds with the image permutation on the
  // per-lane SOURCE address — piece j of a unit covers unit-image bytes
  // [j*8192 + tid*16], whose content is the global chunk img_inv() decodes.
  // The source pointers walk down the chunk 32 rows per issued unit.
  const bf16* pdz[2];
  const bf16* px[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int gm, gc;
    img_inv(j * 8192 + tid * 16, gm, gc);
    if constexpr (RAGGED) {
      // past a ragged edge: the row's last in-range chunk (header)
      const int cn = n0 + gc < N ? n0 + gc : N - 8;
      const int ck = k0 + gc < Kw ? k0 + gc : Kw - 8;
      pdz[j] = DZ + (m_begin + gm) * N + cn;
      px[j] = X + (m_begin + gm) * Kw + ck;
    } else {
      pdz[j] = DZ + (m_begin + gm) * N + n0 + gc;
      px[j] = X + (m_begin + gm) * Kw + k0 + gc;
    }
  }
  const int ldst16 = tid * 16;
  auto issue_unit = [&](char* slot) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      glds16(pdz[j], slot + j * 8192 + ldst16);
      pdz[j] += (int64_t)BMU * N;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      glds16(px[j], slot + UNIT_BYTES + j * 8192 + ldst16);
      px[j] += (int64_t)BMU * Kw;
    }
  };

  typedef short s8 __attribute__((ext_vector_type(8)));
  // Tail-tile staging into slots 0 (rows 0..31) and 1 (rows 32..63):
  // coalesced guarded loads (zero-filled out of range) + scattered LDS
  // writes; round-by-round to keep register pressure low — it runs once.
  auto stage_reg_tail = [&]() {
    const int64_t mt0 = m_begin + (int64_t)nfull * BMS;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int g = r * NTHREADS + tid;
      const int m_loc = g >> 5, col = (g & 31) * 8;
      const int64_t m = mt0 + m_loc;
      s8 a = s8{}, b = s8{};
      if constexpr (RAGGED) {
        // columns clamped as in the ring, rows still zero-filled
        if (m < m_end) {
          a = *reinterpret_cast<const s8*>(DZ + m * N + (n0 + col < N ? n0 + col : N - 8));
          b = *reinterpret_cast<const s8*>(X + m * Kw + (k0 + col < Kw ? k0 + col : Kw - 8));
        }
      } else if (m < m_end) {
        a = *reinterpret_cast<const s8*>(DZ + m * N + n0 + col);
        b = *reinterpret_cast<const s8*>(X + m * Kw + k0 + col);
      }
      char* slot = smem + (m_loc >> 5) * SLOT_BYTES + img_off(m_loc & 31, col);
      *reinterpret_cast<s8*>(slot) = a;
      *reinterpret_cast<s8*>(slot + UNIT_BYTES) = b;
    }
  };

  // Per-lane tr-read address term: lane*8 B — each lane points at its own
  // consecutive b64 slot; the hardware transposes within each 16-lane group
  // (verified by ext.tr16_probe mode 1: lane l elem j reads short
  // (l>>4)*64 + (l&15) + j*16 relative to lane 0's address).
  const int lane_term = lane * 8;

  // RAGGED + DBOUT: a wave whose sub-block pr is dead only because its
  // k-columns lie beyond Kw still owns its share of the bias fold (fold_rd[pr]:
  // its 16 fold columns start inside N).  It reads the one dz fragment it
  // folds, mi = wn, retired by the lgkmcnt(0) of the same asm like every other
  // read of the unit (WAR, header).
  bool fold_rd[2] = {false, false};
  if constexpr (RAGGED && DBOUT) {
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int nf = n0 + (wv >> 2) * 64 + 16 * (wv & 3);
    fold_rd[0] = !live[0] && nf < N;
    fold_rd[1] = !live[1] && nf + 128 < N;
  }
  auto fold_only = [&](const char* slot, int pr) __attribute__((always_inline)) {
    typedef const __attribute__((address_space(3))) char* lds_p;
    const lds_p p =
        (lds_p)(const void*)(slot + pr * 8192 + wm * 4096 + wn * 1024 + lane_term);
    bf16x4_t l, h;
    asm volatile(
        "ds_read_b64_tr_b16 %0, %2 offset:0\n\t"
        "ds_read_b64_tr_b16 %1, %2 offset:512\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(l), "=&v"(h)
        : "v"(p)
        : "memory");
    db_acc[pr] += sum8(__builtin_shufflevector(l, h, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  // One unit = phases A (pr=0) and B (pr=1).  before_bb runs ahead of the
  // barrier of phase B, after_bb right behind it (the ring's wait / issue
  // points; empty for the tail).
  auto consume_unit = [&](const char* slot, auto&& before_bb,
                          auto&& after_bb) __attribute__((always_inline)) {
    typedef const __attribute__((address_space(3))) char* lds_p;
    bf16x8_t xb[4];  // X-side fragments, reused across the pr pair
    bool do_fold = false;
    if (DBOUT) {
      do_fold = unit_no == fold_at;
      if (do_fold) fold_at += fold_p;
      ++unit_no;
    }
    // ---------- phase A (pr=0) ----------
    if (RAGGED && !live[0]) {
      // live[1] implies live[0]: no X fragments are needed either
      if (DBOUT && do_fold && fold_rd[0]) fold_only(slot, 0);
      raw_barrier();
    } else {
      // B (X image) frags ni=0..3 at nt = wn*4+ni, plus A (dz) frags
      // mi=0..3 at nt = wm*4+mi (pr=0).  8+8 tr reads + lgkmcnt(0) in one
      // asm (form i).
      const lds_p bxi = (lds_p)(const void*)(slot + UNIT_BYTES + wn * 4096 + lane_term);
      const lds_p adi = (lds_p)(const void*)(slot + wm * 4096 + lane_term);
      bf16x4_t b0l, b0h, b1l, b1h, b2l, b2h, b3l, b3h;
      bf16x4_t a0l, a0h, a1l, a1h, a2l, a2h, a3l, a3h;
      asm volatile(
          "ds_read_b64_tr_b16 %0, %16 offset:0\n\t"
          "ds_read_b64_tr_b16 %1, %16 offset:512\n\t"
          "ds_read_b64_tr_b16 %2, %16 offset:1024\n\t"
          "ds_read_b64_tr_b16 %3, %16 offset:1536\n\t"
          "ds_read_b64_tr_b16 %4, %16 offset:2048\n\t"
          "ds_read_b64_tr_b16 %5, %16 offset:2560\n\t"
          "ds_read_b64_tr_b16 %6, %16 offset:3072\n\t"
          "ds_read_b64_tr_b16 %7, %16 offset:3584\n\t"
          "ds_read_b64_tr_b16 %8, %17 offset:0\n\t"
          "ds_read_b64_tr_b16 %9, %17 offset:512\n\t"
          "ds_read_b64_tr_b16 %10, %17 offset:1024\n\t"
          "ds_read_b64_tr_b16 %11, %17 offset:1536\n\t"
          "ds_read_b64_tr_b16 %12, %17 offset:2048\n\t"
          "ds_read_b64_tr_b16 %13, %17 offset:2560\n\t"
          "ds_read_b64_tr_b16 %14, %17 offset:3072\n\t"
          "ds_read_b64_tr_b16 %15, %17 offset:3584\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(b0l), "=&v"(b0h), "=&v"(b1l), "=&v"(b1h), "=&v"(b2l), "=&v"(b2h),
            "=&v"(b3l), "=&v"(b3h), "=&v"(a0l), "=&v"(a0h), "=&v"(a1l), "=&v"(a1h),
            "=&v"(a2l), "=&v"(a2h), "=&v"(a3l), "=&v"(a3h)
          : "v"(bxi), "v"(adi)
          : "memory");
      __builtin_amdgcn_sched_barrier(0);
      xb[0] = __builtin_shufflevector(b0l, b0h, 0, 1, 2, 3, 4, 5, 6, 7);
      xb[1] = __builtin_shufflevector(b1l, b1h, 0, 1, 2, 3, 4, 5, 6, 7);
      xb[2] = __builtin_shufflevector(b2l, b2h, 0, 1, 2, 3, 4, 5, 6, 7);
      xb[3] = __builtin_shufflevector(b3l, b3h, 0, 1, 2, 3, 4, 5, 6, 7);
      bf16x8_t ad[4];
      ad[0] = __builtin_shufflevector(a0l, a0h, 0, 1, 2, 3, 4, 5, 6, 7);
      ad[1] = __builtin_shufflevector(a1l, a1h, 0, 1, 2, 3, 4, 5, 6, 7);
      ad[2] = __builtin_shufflevector(a2l, a2h, 0, 1, 2, 3, 4, 5, 6, 7);
      ad[3] = __builtin_shufflevector(a3l, a3h, 0, 1, 2, 3, 4, 5, 6, 7);
      if (DBOUT && do_fold) fold(ad, 0);
      raw_barrier();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[0][mi][ni] = MFMA16(ad[mi], xb[ni], acc[0][mi][ni]);
      __builtin_amdgcn_s_setprio(0);
    }
    // ---------- phase B (pr=1) ----------
    if (RAGGED && !live[1]) {
      if (DBOUT && do_fold && fold_rd[1]) fold_only(slot, 1);
      before_bb();
      raw_barrier();
      after_bb();
    } else {
      const lds_p adi = (lds_p)(const void*)(slot + 8192 + wm * 4096 + lane_term);
      bf16x4_t a0l, a0h, a1l, a1h, a2l, a2h, a3l, a3h;
      asm volatile(
          "ds_read_b64_tr_b16 %0, %8 offset:0\n\t"
          "ds_read_b64_tr_b16 %1, %8 offset:512\n\t"
          "ds_read_b64_tr_b16 %2, %8 offset:1024\n\t"
          "ds_read_b64_tr_b16 %3, %8 offset:1536\n\t"
          "ds_read_b64_tr_b16 %4, %8 offset:2048\n\t"
          "ds_read_b64_tr_b16 %5, %8 offset:2560\n\t"
          "ds_read_b64_tr_b16 %6, %8 offset:3072\n\t"
          "ds_read_b64_tr_b16 %7, %8 offset:3584\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(a0l), "=&v"(a0h), "=&v"(a1l), "=&v"(a1h), "=&v"(a2l), "=&v"(a2h),
            "=&v"(a3l), "=&v"(a3h)
          : "v"(adi)
          : "memory");
      __builtin_amdgcn_sched_barrier(0);
      bf16x8_t ad[4];
      ad[0] = __builtin_shufflevector(a0l, a0h, 0, 1, 2, 3, 4, 5, 6, 7);
      ad[1] = __builtin_shufflevector(a1l, a1h, 0, 1, 2, 3, 4, 5, 6, 7);
      ad[2] = __builtin_shufflevector(a2l, a2h, 0, 1, 2, 3, 4, 5, 6, 7);
      ad[3] = __builtin_shufflevector(a3l, a3h, 0, 1, 2, 3, 4, 5, 6, 7);
      if (DBOUT && do_fold) fold(ad, 1);
      before_bb();
      raw_barrier();
      after_bb();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[1][mi][ni] = MFMA16(ad[mi], xb[ni], acc[1][mi][ni]);
      __builtin_amdgcn_s_setprio(0);
    }
  };

  if (nunit > 0) {
    // prologue: fill the ring, certify unit 0
    const int npro = nunit < RING ? nunit : RING;
    for (int u = 0; u < npro; ++u) issue_unit(smem + u * SLOT_BYTES);
    wait_units_in_flight(npro - 1);
    raw_barrier();
    int slot = 0;
    for (int u = 0; u < nunit; ++u) {
      char* sp = smem + slot * SLOT_BYTES;
      consume_unit(
          sp,
          [&] {  // certify unit u+1: units u+2 .. min(u+RING-1, last) stay in flight
            if (u + 1 < nunit) {
              const int behind = nunit - 2 - u;
              wait_units_in_flight(behind < RING - 2 ? behind : RING - 2);
            }
          },
          [&] {
            if (u + RING < nunit) issue_unit(sp);
          });
      slot = slot + 1 == RING ? 0 : slot + 1;
    }
  }
  if (tail) {
    // the ring is drained and every slot is free (see header)
    stage_reg_tail();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    raw_barrier();
    for (int kh = 0; kh < 2; ++kh)
      consume_unit(smem + kh * SLOT_BYTES, [] {}, [] {});
  }

  if (DBOUT && kt < fold_p) {
    // A-frag row for lane = lo: db_acc[pr] covers n = n0 + pr*128 + wm*64 +
    // 16*wn + lo over the 8-row groups (hi) of the units this wave folded;
    // reduce over hi, one atomic per n per folding k-tile per split
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      float v_ = db_acc[pr];
      v_ += __shfl_xor(v_, 16, WAVE);
      v_ += __shfl_xor(v_, 32, WAVE);
      if (hi == 0 && (!RAGGED || n0 + pr * 128 + wm * 64 + 16 * wn + lo < N))
        atomicAdd(DB + n0 + pr * 128 + wm * 64 + 16 * wn + lo, v_);
    }
  }

  // Epilogue: acc[pr][mi][ni] -> C rows n = n0 + pr*128 + wm*64 + 16mi +
  // hi*4 + r, cols k = k0 + wn*64 + 16ni + lo.
#pragma unroll
  for (int pr = 0; pr < 2; ++pr)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + pr * 128 + wm * 64 + 16 * mi + hi * 4 + r;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          const int k = k0 + wn * 64 + 16 * ni + lo;
          // WSOUT: each split owns a private C slice (no atomics; a reduce
          // kernel folds the splits)
          float* dst = C + (WSOUT ? (int64_t)blockIdx.y * N * Kw : 0) +
                       (int64_t)n * Kw + k;
          if (!RAGGED || (n < N && k < Kw)) *dst = acc[pr][mi][ni][r];
        }
      }
}

// Folds the per-split fp32 slices in fixed order; BF16OUT rounds the fp32
// sum once on the way out (bitwise what a separate fp32 -> bf16 cast of
// the fp32 result gives).
template <bool BF16OUT>
__global__ void ws_reduce_kernel(const float* __restrict__ ws, void* __restrict__ out,
                                 int64_t n, int splits) {
  typedef float f32x4_r __attribute__((ext_vector_type(4)));
  const int64_t nv = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
       i += (int64_t)gridDim.x * blockDim.x) {
    f32x4_r acc = *reinterpret_cast<const f32x4_r*>(ws + i * 4);
    for (int sp = 1; sp < splits; ++sp) {
      const f32x4_r v = *reinterpret_cast<const f32x4_r*>(ws + (int64_t)sp * n + i * 4);
      acc += v;
    }
    if (BF16OUT) {
      bf16x4_t o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = f2bfs(acc[j]);
      *reinterpret_cast<bf16x4_t*>(reinterpret_cast<bf16*>(out) + i * 4) = o;
    } else {
      *reinterpret_cast<f32x4_r*>(reinterpret_cast<float*>(out) + i * 4) = acc;
    }
  }
}

}  // namespace

bool gemm_tn8p_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && (N % BN == 0) && (K % BKW == 0);
}

// Split-M count for `tiles` output tiles on `cus` compute units (one
// workgroup per CU: the ring takes the whole LDS).  The grid runs in
// ceil(tiles*s/cus) rounds of ceil(M/s/64) m-steps each; pick the s in
// [1, 24] (or up to cus/tiles, so that few-tile shapes can still fill one
// round) with the least rounds x steps, the smaller s on a tie (fewer
// workspace slices to write and fold).  Costs within 5% of the least count
// as a tie: the model is no finer than that (36 tiles at M=201728: s=21
// models 4.6% under s=20 and measures 1.5% ahead on fc1, 2.5% behind on
// fc2).  A chunk is capped at MAX_CHUNK_STEPS m-steps where the split
// limit allows it: the round model assumes workgroups of equal speed, and
// one round of very long chunks cannot be rebalanced by the dispatcher
// (fc2 dW of ViT-B, 36 tiles: 1 round x 451 steps measured 7% behind 3
// rounds x 158 steps; profiles/dw_pipeline_NOTES.md).
int64_t gemm_tn8p_choose_splitm(int64_t M, int64_t tiles, int64_t cus) {
  constexpr int64_t MAX_CHUNK_STEPS = 192;
  const int64_t msteps = (M + BMS - 1) / BMS;
  const int64_t smax =
      std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(24, cus / tiles), msteps));
  const int64_t smin =
      std::min<int64_t>(smax, (msteps + MAX_CHUNK_STEPS - 1) / MAX_CHUNK_STEPS);
  auto cost = [&](int64_t s) {
    const int64_t rounds = (tiles * s + cus - 1) / cus;
    const int64_t steps = ((M + s - 1) / s + BMS - 1) / BMS;
    return rounds * steps;
  };
  int64_t least = cost(smin);
  for (int64_t s = smin + 1; s <= smax; ++s) least = std::min(least, cost(s));
  for (int64_t s = smin; s <= smax; ++s)
    if (cost(s) * 20 <= least * 21) return s;
  return smax;
}

// out[i] = sum over `splits` fp32 slices of n elements each (n % 4 == 0), in
// fixed order, as fp32 or rounded once to bf16. Shared with gemm_tn128.hip.
void tn_ws_reduce(const float* ws, void* out, int64_t n, int splits, bool out_bf16,
                  hipStream_t stream) {
  const int block = 256;
  const int grid = (int)std::min<int64_t>((n / 4 + block - 1) / block, 8192);
  if (out_bf16)
    hipLaunchKernelGGL(ws_reduce_kernel<true>, dim3(grid), dim3(block), 0, stream, ws, out, n,
                       splits);
  else
    hipLaunchKernelGGL(ws_reduce_kernel<false>, dim3(grid), dim3(block), 0, stream, ws, out, n,
                       splits);
}

// Domain of the RAGGED instantiations: the 128-tile kernel's.
bool gemm_tn8p_ragged_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0 && N <= INT_MAX &&
         K <= INT_MAX;
}

template <bool RAGGED>
static torch::Tensor tn8p_run(torch::Tensor dz, torch::Tensor x, float* dbp, int64_t splitm_arg,
                              bool out_bf16,
                              const c10::optional<torch::Tensor>& out = c10::nullopt) {
  // dz (M, N) bf16, x (M, Kw) bf16 -> dW (N, Kw) = dz^T @ x, fp32 or
  // (out_bf16) the fp32 result rounded once to bf16
  // (dbp != nullptr: also fold db[n] = colsum(dz) out of the A fragments)
  // (out, RAGGED only: the fp32 (N, Kw) tensor the result is written to)
  TORCH_CHECK(dz.is_cuda() && dz.is_contiguous() && x.is_contiguous());
  TORCH_CHECK(dz.scalar_type() == torch::kBFloat16 && x.scalar_type() == torch::kBFloat16);
  if (RAGGED) {
    TORCH_CHECK(x.is_cuda() && dz.dim() == 2 && x.dim() == 2);
    TORCH_CHECK(x.size(0) == dz.size(0) &&
                    gemm_tn8p_ragged_supported(dz.size(0), dz.size(1), x.size(1)),
                "gemm_tn_8p_ragged: needs M >= 1 and N, K multiples of 8, got M=", dz.size(0),
                " N=", dz.size(1), " K=", x.size(1));
    TORCH_CHECK(reinterpret_cast<uintptr_t>(dz.data_ptr()) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
                "gemm_tn_8p_ragged: operands must be 16-byte aligned");
  }
  const int64_t M = dz.size(0);
  const int N = dz.size(1), Kw = x.size(1);
  TORCH_CHECK(x.size(0) == M && (RAGGED || gemm_tn8p_supported(M, N, Kw)));
  TORCH_CHECK(splitm_arg >= 0, "splitm must be >= 0 (0 = heuristic)");
  if (out.has_value()) {
    TORCH_CHECK(RAGGED && !out_bf16 && out->is_cuda() && out->is_contiguous() &&
                    out->scalar_type() == torch::kFloat32 && out->dim() == 2 &&
                    out->size(0) == N && out->size(1) == Kw &&
                    reinterpret_cast<uintptr_t>(out->data_ptr()) % 16 == 0,
                "gemm_tn_8p_ragged: out must be a contiguous 16-byte-aligned fp32 (N, K) "
                "tensor, without out_bf16");
  }
  auto stream = at::hip::getCurrentHIPStream();
  const int64_t tiles64 =
      RAGGED ? (int64_t)((N + BN - 1) / BN) * ((Kw + BKW - 1) / BKW) : (N / BN) * (Kw / BKW);
  TORCH_CHECK(tiles64 <= INT_MAX, "gemm_tn_8p: too many output tiles");
  const int tiles = (int)tiles64;
  // split count: the splitm argument, else JIMM_AMD_DW_SPLITM (read once,
  // for tuning), else the round-aware choice above
  static const int splitm_env = [] {
    const char* e = getenv("JIMM_AMD_DW_SPLITM");
    return e ? atoi(e) : 0;
  }();
  const int64_t msteps = (M + BMS - 1) / BMS;
  int64_t want = splitm_arg > 0 ? splitm_arg : splitm_env;
  if (want <= 0)
    want = gemm_tn8p_choose_splitm(M, tiles,
                                   at::cuda::getCurrentDeviceProperties()->multiProcessorCount);
  int splitm = (int)std::max<int64_t>(1, std::min<int64_t>(want, msteps));
  int64_t chunk = ((M + splitm - 1) / splitm + BMS - 1) / BMS * BMS;
  splitm = (int)((M + chunk - 1) / chunk);
  TORCH_CHECK(!RAGGED || splitm <= 65535, "gemm_tn_8p_ragged: too many splits");
  // More than one split: each writes a private C slice of a workspace and a
  // vectorized reduce folds them in fixed order, so the whole dW is
  // deterministic (measured 662-745 -> 684-824 TF/s over an fp32 atomic
  // combine on the block shapes, profiles/r02_NOTES.md). One split stores
  // straight into an fp32 C.
  const bool use_ws = splitm > 1;
  const auto f32 = dz.options().dtype(torch::kFloat32);
  torch::Tensor C, ws;
  if (use_ws) {
    ws = torch::empty({(int64_t)splitm, (int64_t)N, (int64_t)Kw}, f32);
    C = out.has_value() ? *out
                        : torch::empty({(int64_t)N, (int64_t)Kw}, out_bf16 ? dz.options() : f32);
  } else {
    C = out.has_value() ? *out : torch::empty({(int64_t)N, (int64_t)Kw}, f32);
  }
  const size_t shmem = (size_t)RING * SLOT_BYTES;  // 160 KiB
#define LAUNCH_TN(DBO, WSO)                                                                \
  launch_lds<gemm_tn_8p_kernel<DBO, WSO, RAGGED>>(                                         \
      dim3(tiles, splitm), dim3(NTHREADS), shmem, shmem, stream,                           \
      reinterpret_cast<const bf16*>(dz.data_ptr()),                                        \
      reinterpret_cast<const bf16*>(x.data_ptr()),                                         \
      WSO ? ws.data_ptr<float>() : C.data_ptr<float>(), M, N, Kw, chunk, dbp)
  if (!use_ws) {
    if (dbp) LAUNCH_TN(true, false);
    else LAUNCH_TN(false, false);
    return out_bf16 ? C.to(torch::kBFloat16) : C;
  }
  if (dbp) LAUNCH_TN(true, true);
  else LAUNCH_TN(false, true);
#undef LAUNCH_TN
  tn_ws_reduce(ws.data_ptr<float>(), C.data_ptr(), (int64_t)N * Kw, splitm, out_bf16, stream);
  return C;
}

torch::Tensor gemm_tn_8p(torch::Tensor dz, torch::Tensor x, int64_t splitm, bool out_bf16) {
  return tn8p_run<false>(dz, x, nullptr, splitm, out_bf16);
}

std::vector<torch::Tensor> gemm_tn_8p_db(torch::Tensor dz, torch::Tensor x, int64_t splitm,
                                         bool out_bf16) {
  // fused dW + bias-grad: {dW (N, Kw) fp32 or bf16, db (N) fp32}
  auto db = torch::zeros({dz.size(1)}, dz.options().dtype(torch::kFloat32));
  auto C = tn8p_run<false>(dz, x, db.data_ptr<float>(), splitm, out_bf16);
  return {C, db};
}

// The same two off the 256 grid (any N % 8 == 0, Kw % 8 == 0): the RAGGED
// instantiations. out: an fp32 (N, Kw) tensor to write dW to instead of a new
// one (a single split stores straight into it).
torch::Tensor gemm_tn_8p_ragged(torch::Tensor dz, torch::Tensor x, int64_t splitm, bool out_bf16,
                                c10::optional<torch::Tensor> out) {
  return tn8p_run<true>(dz, x, nullptr, splitm, out_bf16, out);
}

std::vector<torch::Tensor> gemm_tn_8p_ragged_db(torch::Tensor dz, torch::Tensor x,
                                                int64_t splitm, bool out_bf16,
                                                c10::optional<torch::Tensor> out) {
  TORCH_CHECK(dz.is_cuda() && dz.dim() == 2);
  auto db = torch::zeros({dz.size(1)}, dz.options().dtype(torch::kFloat32));
  auto C = tn8p_run<true>(dz, x, db.data_ptr<float>(), splitm, out_bf16, out);
  return {C, db};
}
