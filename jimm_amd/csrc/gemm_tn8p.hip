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
// Split-M: grid.y walks m-chunks (slow index -> the chunk's operand rows
// stay L3-resident across its output tiles).  Each split writes a private
// fp32 slice of a workspace and ws_reduce_kernel folds them in fixed order
// (deterministic), writing fp32 or bf16; grid.y == 1 stores once, straight
// into C.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

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

template <bool DBOUT, bool WSOUT>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_tn_8p_kernel(
    const bf16* __restrict__ DZ, const bf16* __restrict__ X, float* __restrict__ C,
    int64_t M, int N, int Kw, int64_t chunk_m, float* __restrict__ DB) {
  // ring slot s at s*32 KiB: dz unit image at +0, X unit image at +16 KiB
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wave = tid / WAVE;
  const int lo = lane & 15, hi = lane >> 4;

  const int nt_n = N / BN, nt_k = Kw / BKW;
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

  f32x4_t acc[2][4][4] = {};  // [pr][mi][ni]
  // DBOUT: db[n] = sum_m dz[m][n] folded out of the A fragments already in
  // registers (the separate colsum kernel re-reads dz from HBM). Only the
  // k0==0 / wn==0 waves contribute (the same dz fragments are read by every
  // k-tile and every wn), so the whole-M coverage comes from the k0==0
  // column of workgroups across splits.
  float db_acc[2][4] = {};

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
    pdz[j] = DZ + (m_begin + gm) * N + n0 + gc;
    px[j] = X + (m_begin + gm) * Kw + k0 + gc;
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
      if (m < m_end) {
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

  // One unit = phases A (pr=0) and B (pr=1).  before_bb runs ahead of the
  // barrier of phase B, after_bb right behind it (the ring's wait / issue
  // points; empty for the tail).
  auto consume_unit = [&](const char* slot, auto&& before_bb,
                          auto&& after_bb) __attribute__((always_inline)) {
    typedef const __attribute__((address_space(3))) char* lds_p;
    bf16x8_t xb[4];  // X-side fragments, reused across the pr pair
    // ---------- phase A (pr=0) ----------
    {
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
      if (DBOUT && wn == 0 && k0 == 0) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          const bf16* av = reinterpret_cast<const bf16*>(&ad[mi]);
          float s8 = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) s8 += bf2f(av[j]);
          db_acc[0][mi] += s8;
        }
      }
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
    {
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
      if (DBOUT && wn == 0 && k0 == 0) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          const bf16* av = reinterpret_cast<const bf16*>(&ad[mi]);
          float s8 = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) s8 += bf2f(av[j]);
          db_acc[1][mi] += s8;
        }
      }
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

  if (DBOUT && wn == 0 && k0 == 0) {
    // A-frag row for lane = lo: db_acc[pr][mi] covers n = n0 + pr*128 +
    // wm*64 + 16*mi + lo over this wave's m chunks (hi groups); reduce
    // over hi, one atomic per n per split
#pragma unroll
    for (int pr = 0; pr < 2; ++pr)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        float v_ = db_acc[pr][mi];
        v_ += __shfl_xor(v_, 16, WAVE);
        v_ += __shfl_xor(v_, 32, WAVE);
        if (hi == 0) atomicAdd(DB + n0 + pr * 128 + wm * 64 + 16 * mi + lo, v_);
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
          *dst = acc[pr][mi][ni][r];
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

static torch::Tensor tn8p_run(torch::Tensor dz, torch::Tensor x, float* dbp, int64_t splitm_arg,
                              bool out_bf16) {
  // dz (M, N) bf16, x (M, Kw) bf16 -> dW (N, Kw) = dz^T @ x, fp32 or
  // (out_bf16) the fp32 result rounded once to bf16
  // (dbp != nullptr: also fold db[n] = colsum(dz) out of the A fragments)
  TORCH_CHECK(dz.is_cuda() && dz.is_contiguous() && x.is_contiguous());
  TORCH_CHECK(dz.scalar_type() == torch::kBFloat16 && x.scalar_type() == torch::kBFloat16);
  const int64_t M = dz.size(0);
  const int N = dz.size(1), Kw = x.size(1);
  TORCH_CHECK(x.size(0) == M && gemm_tn8p_supported(M, N, Kw));
  TORCH_CHECK(splitm_arg >= 0, "splitm must be >= 0 (0 = heuristic)");
  auto stream = at::hip::getCurrentHIPStream();
  const int tiles = (N / BN) * (Kw / BKW);
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
    C = torch::empty({(int64_t)N, (int64_t)Kw}, out_bf16 ? dz.options() : f32);
  } else {
    C = torch::empty({(int64_t)N, (int64_t)Kw}, f32);
  }
  const size_t shmem = (size_t)RING * SLOT_BYTES;  // 160 KiB
#define LAUNCH_TN(DBO, WSO)                                                                \
  launch_lds<gemm_tn_8p_kernel<DBO, WSO>>(                                                 \
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
  const int64_t n = (int64_t)N * Kw;
  const int block = 256;
  const int grid = (int)std::min<int64_t>((n / 4 + block - 1) / block, 8192);
  if (out_bf16)
    hipLaunchKernelGGL(ws_reduce_kernel<true>, dim3(grid), dim3(block), 0, stream,
                       ws.data_ptr<float>(), C.data_ptr(), n, splitm);
  else
    hipLaunchKernelGGL(ws_reduce_kernel<false>, dim3(grid), dim3(block), 0, stream,
                       ws.data_ptr<float>(), C.data_ptr(), n, splitm);
  return C;
}

torch::Tensor gemm_tn_8p(torch::Tensor dz, torch::Tensor x, int64_t splitm, bool out_bf16) {
  return tn8p_run(dz, x, nullptr, splitm, out_bf16);
}

std::vector<torch::Tensor> gemm_tn_8p_db(torch::Tensor dz, torch::Tensor x, int64_t splitm,
                                         bool out_bf16) {
  // fused dW + bias-grad: {dW (N, Kw) fp32 or bf16, db (N) fp32}
  auto db = torch::zeros({dz.size(1)}, dz.options().dtype(torch::kFloat32));
  auto C = tn8p_run(dz, x, db.data_ptr<float>(), splitm, out_bf16);
  return {C, db};
}
