// TN weight-gradient GEMM for weight shapes off the 256 grid:
// dW[N,Kw] = dz^T @ X, 128x128 output tiles, ragged N and Kw, split-M, MFMA
// bf16.  The 256-tile kernel (gemm_tn8p.hip) needs N % 256 == 0 and
// Kw % 256 == 0; this one takes any N % 8 == 0, Kw % 8 == 0 (ViT-S/Ti 384 /
// 192, so400m 1152 / 3456 / 4304, class heads 1000 / 10, projections 640).
// Which of those shapes reach it is the rule of gemm_dw_db
// (ops/hip_linear.py).
//
// N and Kw are OUTPUT dimensions of this GEMM, so a ragged edge needs no zero
// fill: a staging lane whose 8-column chunk starts at or beyond N (Kw) reads
// the chunk at N - 8 (Kw - 8) instead — a valid, 16-byte-aligned address of
// the same row — and what it brings in lands only in accumulator rows /
// columns that the epilogue and the bias fold never store (both predicate on
// n < N, k < Kw).  global_load_lds staging survives unchanged.
//
// Tile and waves: 256 threads, four waves laid out 2 (wm: n) x 2 (wn: k),
// each owning 64 x 64 = acc[4][4] of f32x4 on v_mfma_f32_16x16x32_bf16.  The
// m-step is 64 rows in two 32-row units, as in the 256-tile kernel.
//
// Unit image (8 KiB per operand, 32 m x 128 columns): the 256-tile kernel's
// byte formula with nt = col >> 4 in 0..7,
//   byte(m, col) = nt*1024 + qpos*128 + jm*32 + u*16
//   q' = (m>>2)&7, jm = m&3, qpos = (q'&1)*4 + (q'>>1), u = (col>>3)&1,
// filled by glds16 with the inverse permutation on the per-lane SOURCE
// address (2 glds per operand per thread and unit: 4 per unit, the counted
// vmcnt literals of the 256-tile kernel carry over) and read back with
// ds_read_b64_tr_b16 at base + lane*8 (+512 for the odd m-quads).
//
// Ring: a slot is 16 KiB (dz image at +0, X image at +8 KiB), RING = 5 slots
// are 80 KiB, so TWO workgroups share a CU (the 256-tile kernel takes the
// whole LDS for one): one workgroup's barrier and fragment reads run under
// the other's MFMAs.  Unit u lives in slot u % RING.  A wave needs all 4 dz
// and all 4 X fragments of a unit for its 16 MFMAs and there are no
// row-halves to alternate, so a unit is ONE phase with one raw s_barrier:
//   P(u): 8 + 8 tr-reads of slot(u); lgkmcnt(0); [bias fold]; counted
//         vmcnt; barrier B(u); issue unit u+RING into slot(u); 16 MFMA
//         under s_setprio(1)
// Certification:
//   RAW  unit v is first read in P(v), after barrier B(v-1).  Before
//        arriving at B(v-1) every wave waits until its own pieces of v have
//        landed: it has issued units up to v+RING-2 by then and vmcnt
//        retires loads in order, so s_waitcnt vmcnt(4*(RING-2)) (fewer newer
//        units near the end of the stream: 4*(units still behind v), 0 only
//        for the last unit) covers v.  B(v-1) then makes all waves' pieces
//        visible.  The prologue issues units 0..RING-1, waits down to unit 0
//        the same way and raises one barrier before P(0).
//   WAR  slot(u) is rewritten by unit u+RING, issued after B(u).  Every
//        wave's reads of unit u are retired by the lgkmcnt(0) of P(u)'s asm
//        block, i.e. before the wave arrives at B(u); a glds issued after
//        B(u) cannot overtake them.
//   So RING-1 units (2 tiles) are in flight across barriers and no wave
//   drains the queue inside the loop.  The counted wait is exact because the
//   loop holds no other vector-memory instruction.
// Ragged M: a last tile with fewer than 64 rows is staged after the ring has
// drained (the last unit's wait is vmcnt(0) and B(last) has passed, so every
// slot is free): guarded register loads (zero rows beyond the chunk, zero
// chunks beyond N / Kw), ds_write_b128 into slots 0 / 1, one barrier, the
// same walk.
//
// Bias fold (DBOUT), dealt out as in the 256-tile kernel: the two waves of
// equal wm hold the same dz fragments, so wave (wm, wn) folds fragments
// mi in {2*wn, 2*wn + 1}, and of a chunk's 32-row units k-tile kt folds
// those with unit % P == kt, P = min(ceil(Kw/128), FOLD_PMAX).  A folding
// wave ends with one fp32 atomic per valid column.
//
// Split-M and combine: as the 256-tile kernel (grid.y walks m-chunks, each
// split writes a private fp32 workspace slice, tn_ws_reduce folds them in
// fixed order; one split stores straight into C).  dW is bitwise
// deterministic.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <climits>

#include "mfma.h"

// gemm_tn8p.hip
int64_t gemm_tn8p_choose_splitm(int64_t M, int64_t tiles, int64_t cus);
void tn_ws_reduce(const float* ws, void* out, int64_t n, int splits, bool out_bf16,
                  hipStream_t stream);

namespace {

typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef short bf16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int BN = 128, BKW = 128, BMS = 64;  // n-tile, k-tile, m-step
constexpr int NTHREADS = 256;
constexpr int BMU = 32;            // m-rows per staging unit
constexpr int UNIT_BYTES = 8192;   // one operand's 32x128 bf16 unit image
constexpr int SLOT_BYTES = 2 * UNIT_BYTES;  // dz image + X image
constexpr int RING = 5;            // ring slots (RING * 16 KiB of LDS)
constexpr int GLDS_PER_UNIT = 4;   // per thread: 2 dz + 2 X
constexpr int FOLD_PMAX = 4;       // k-tiles of one n-tile that share the bias fold
constexpr int WG_PER_CU = 2;       // 2 x 80 KiB of LDS

// fp32 arithmetic (the bias fold's sums) is not to be packed in pairs
// (v_pk_*_f32) in this file: the device pass compiles every function and
// lambda below without the feature.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

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

// unit-image byte offset of element (m_local 0..31, col 0..127)
__device__ __forceinline__ int img_off(int m, int col) {
  const int q = (m >> 2) & 7, jm = m & 3;
  const int qpos = (q & 1) * 4 + (q >> 1);
  return (col >> 4) * 1024 + qpos * 128 + jm * 32 + ((col >> 3) & 1) * 16;
}

// inverse: unit-image byte offset o (16-B granular) -> (m_local, col)
__device__ __forceinline__ void img_inv(int o, int& m, int& col) {
  const int nt = (o >> 10) & 7;
  const int qpos = (o >> 7) & 7;
  const int jm = (o >> 5) & 3;
  const int u = (o >> 4) & 1;
  const int q = ((qpos >> 2) & 1) + (qpos & 3) * 2;
  m = q * 4 + jm;
  col = nt * 16 + u * 8;
}

template <bool DBOUT, bool WSOUT>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_tn_128_kernel(
    const bf16* __restrict__ DZ, const bf16* __restrict__ X, float* __restrict__ C,
    int64_t M, int N, int Kw, int64_t chunk_m, float* __restrict__ DB) {
  // ring slot s at s*16 KiB: dz unit image at +0, X unit image at +8 KiB
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wave = tid / WAVE;
  const int lo = lane & 15, hi = lane >> 4;

  const int nt_n = (N + BN - 1) / BN, nt_k = (Kw + BKW - 1) / BKW;
  const int wg = xcd_remap(blockIdx.x, nt_n * nt_k);
  const int n0 = (wg / nt_k) * BN;
  const int k0 = (wg % nt_k) * BKW;
  const int wm = wave >> 1;  // 0..1 (n sub-position)
  const int wn = wave & 1;   // 0..1 (k sub-position)

  const int64_t m_begin = (int64_t)blockIdx.y * chunk_m;
  const int64_t m_end = m_begin + chunk_m < M ? m_begin + chunk_m : M;
  if (m_end <= m_begin) return;
  const int nfull = (int)((m_end - m_begin) / BMS);  // full 64-row tiles
  const int nunit = 2 * nfull;                       // ring units
  const bool tail = (m_end - m_begin) % BMS != 0;

  f32x4_t acc[4][4] = {};  // [mi][ni]
  // DBOUT: this wave folds fragments mi = 2*wn, 2*wn + 1 of the units
  // fold_at, fold_at + fold_p, ...; k-tiles >= fold_p never fold (header).
  float db_acc[2] = {};
  const int wn_u = __builtin_amdgcn_readfirstlane(wn);  // scalar, for the branch
  const int kt = wg % nt_k;
  const int fold_p = nt_k < FOLD_PMAX ? nt_k : FOLD_PMAX;
  int fold_at = kt < fold_p ? kt : INT_MAX;  // next unit of the chunk to fold
  int unit_no = 0;                           // ring units, then the tail's two
  // sum of one fragment's 8 dz values (this lane's column, 8 rows)
  auto sum8 = [](const bf16x8_t& a) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      s += __builtin_bit_cast(float, (unsigned int)(unsigned short)a[j] << 16);
    return s;
  };

  // Ring staging for this thread: piece j of a unit covers unit-image bytes
  // [j*4096 + tid*16], whose content is the global chunk img_inv() decodes,
  // clamped into the operand's last 8 columns past a ragged edge (header).
  // The source pointers walk down the chunk 32 rows per issued unit.
  const bf16* pdz[2];
  const bf16* px[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int gm, gc;
    img_inv(j * 4096 + tid * 16, gm, gc);
    const int cn = n0 + gc < N ? n0 + gc : N - 8;
    const int ck = k0 + gc < Kw ? k0 + gc : Kw - 8;
    pdz[j] = DZ + (m_begin + gm) * N + cn;
    px[j] = X + (m_begin + gm) * Kw + ck;
  }
  const int ldst16 = tid * 16;
  auto issue_unit = [&](char* slot) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      glds16(pdz[j], slot + j * 4096 + ldst16);
      pdz[j] += (int64_t)BMU * N;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      glds16(px[j], slot + UNIT_BYTES + j * 4096 + ldst16);
      px[j] += (int64_t)BMU * Kw;
    }
  };

  typedef short s8 __attribute__((ext_vector_type(8)));
  // Tail-tile staging into slots 0 (rows 0..31) and 1 (rows 32..63): guarded
  // loads (zeros beyond the chunk's rows and the operands' columns) +
  // scattered LDS writes, 64 rows x 16 chunks in 4 rounds; it runs once.
  auto stage_reg_tail = [&]() {
    const int64_t mt0 = m_begin + (int64_t)nfull * BMS;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int g = r * NTHREADS + tid;
      const int m_loc = g >> 4, col = (g & 15) * 8;
      const int64_t m = mt0 + m_loc;
      s8 a = s8{}, b = s8{};
      if (m < m_end && n0 + col < N) a = *reinterpret_cast<const s8*>(DZ + m * N + n0 + col);
      if (m < m_end && k0 + col < Kw) b = *reinterpret_cast<const s8*>(X + m * Kw + k0 + col);
      char* slot = smem + (m_loc >> 5) * SLOT_BYTES + img_off(m_loc & 31, col);
      *reinterpret_cast<s8*>(slot) = a;
      *reinterpret_cast<s8*>(slot + UNIT_BYTES) = b;
    }
  };

  // Per-lane tr-read address term: lane*8 B (gemm_tn8p.hip).
  const int lane_term = lane * 8;

  // One unit = one phase.  before_b runs ahead of the barrier, after_b right
  // behind it (the ring's wait / issue points; empty for the tail).
  auto consume_unit = [&](const char* slot, auto&& before_b,
                          auto&& after_b) __attribute__((always_inline)) {
    typedef const __attribute__((address_space(3))) char* lds_p;
    // X frags ni = 0..3 at nt = wn*4 + ni, dz frags mi = 0..3 at
    // nt = wm*4 + mi.  8 + 8 tr reads + lgkmcnt(0) in one asm.
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
    bf16x8_t xb[4], ad[4];
    xb[0] = __builtin_shufflevector(b0l, b0h, 0, 1, 2, 3, 4, 5, 6, 7);
    xb[1] = __builtin_shufflevector(b1l, b1h, 0, 1, 2, 3, 4, 5, 6, 7);
    xb[2] = __builtin_shufflevector(b2l, b2h, 0, 1, 2, 3, 4, 5, 6, 7);
    xb[3] = __builtin_shufflevector(b3l, b3h, 0, 1, 2, 3, 4, 5, 6, 7);
    ad[0] = __builtin_shufflevector(a0l, a0h, 0, 1, 2, 3, 4, 5, 6, 7);
    ad[1] = __builtin_shufflevector(a1l, a1h, 0, 1, 2, 3, 4, 5, 6, 7);
    ad[2] = __builtin_shufflevector(a2l, a2h, 0, 1, 2, 3, 4, 5, 6, 7);
    ad[3] = __builtin_shufflevector(a3l, a3h, 0, 1, 2, 3, 4, 5, 6, 7);
    if (DBOUT) {
      if (unit_no == fold_at) {
        fold_at += fold_p;
        if (wn_u == 0) {
          db_acc[0] += sum8(ad[0]);
          db_acc[1] += sum8(ad[1]);
        } else {
          db_acc[0] += sum8(ad[2]);
          db_acc[1] += sum8(ad[3]);
        }
      }
      ++unit_no;
    }
    before_b();
    raw_barrier();
    after_b();
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = MFMA16(ad[mi], xb[ni], acc[mi][ni]);
    __builtin_amdgcn_s_setprio(0);
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
    // db_acc[j] covers n = n0 + wm*64 + 16*(2*wn + j) + lo over the 8-row
    // groups (hi) of the units this wave folded; reduce over hi, one atomic
    // per valid n per folding k-tile per split.  (Builtins, not the HIP
    // header's __shfl_xor / atomicAdd: those are compiled with packed fp32
    // and would stay out-of-line calls from this file's functions.)
    auto lane_xor = [&](float v, int mask) {
      return __builtin_bit_cast(
          float, __builtin_amdgcn_ds_bpermute((lane ^ mask) << 2, __builtin_bit_cast(int, v)));
    };
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float v_ = db_acc[j];
      v_ += lane_xor(v_, 16);
      v_ += lane_xor(v_, 32);
      const int n = n0 + wm * 64 + 16 * (2 * wn + j) + lo;
      if (hi == 0 && n < N)
        __hip_atomic_fetch_add(DB + n, v_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }

  // Epilogue: acc[mi][ni] -> C rows n = n0 + wm*64 + 16mi + hi*4 + r, cols
  // k = k0 + wn*64 + 16ni + lo, inside the matrix only.  WSOUT: each split
  // owns a private C slice (no atomics; tn_ws_reduce folds the splits).
  float* Cs = C + (WSOUT ? (int64_t)blockIdx.y * N * Kw : 0);
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + wm * 64 + 16 * mi + hi * 4 + r;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int k = k0 + wn * 64 + 16 * ni + lo;
        if (n < N && k < Kw) Cs[(int64_t)n * Kw + k] = acc[mi][ni][r];
      }
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

bool gemm_tn_128_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0 && N <= INT_MAX &&
         K <= INT_MAX;
}

static torch::Tensor tn128_run(torch::Tensor dz, torch::Tensor x, float* dbp,
                               int64_t splitm_arg, bool out_bf16) {
  // dz (M, N) bf16, x (M, Kw) bf16 -> dW (N, Kw) = dz^T @ x, fp32 or
  // (out_bf16) the fp32 result rounded once to bf16
  // (dbp != nullptr: also fold db[n] = colsum(dz) out of the dz fragments)
  TORCH_CHECK(dz.is_cuda() && x.is_cuda() && dz.dim() == 2 && x.dim() == 2);
  TORCH_CHECK(dz.is_contiguous() && x.is_contiguous());
  TORCH_CHECK(dz.scalar_type() == torch::kBFloat16 && x.scalar_type() == torch::kBFloat16);
  const int64_t M = dz.size(0);
  TORCH_CHECK(x.size(0) == M && gemm_tn_128_supported(M, dz.size(1), x.size(1)),
              "gemm_tn_128: needs M >= 1 and N, K multiples of 8, got M=", M,
              " N=", dz.size(1), " K=", x.size(1));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(dz.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "gemm_tn_128: operands must be 16-byte aligned");
  TORCH_CHECK(splitm_arg >= 0, "splitm must be >= 0 (0 = heuristic)");
  const int N = dz.size(1), Kw = x.size(1);
  auto stream = at::hip::getCurrentHIPStream();
  const int64_t tiles64 = (int64_t)((N + BN - 1) / BN) * ((Kw + BKW - 1) / BKW);
  TORCH_CHECK(tiles64 <= INT_MAX, "gemm_tn_128: too many output tiles");
  const int tiles = (int)tiles64;
  // split count: the splitm argument, else the 256-tile kernel's round model
  // over the workgroups the device holds at once (two per CU). A 128-tile
  // m-step is a quarter of the work the model's constants were fitted to;
  // its 5% tie rule and 192-step chunk cap are carried over as they are
  // (the choice measured within 7% of the best of 4 / 8 / 16 / 32 splits on
  // the ViT-S, so400m and class-head shapes; profiles/dw_offgrid_NOTES.md).
  const int64_t msteps = (M + BMS - 1) / BMS;
  int64_t want = splitm_arg;
  if (want <= 0)
    want = gemm_tn8p_choose_splitm(
        M, tiles, (int64_t)WG_PER_CU * at::cuda::getCurrentDeviceProperties()->multiProcessorCount);
  int splitm = (int)std::max<int64_t>(1, std::min<int64_t>(want, msteps));
  const int64_t chunk = ((M + splitm - 1) / splitm + BMS - 1) / BMS * BMS;
  splitm = (int)((M + chunk - 1) / chunk);
  TORCH_CHECK(splitm <= 65535, "gemm_tn_128: too many splits");
  const bool use_ws = splitm > 1;
  const auto f32 = dz.options().dtype(torch::kFloat32);
  torch::Tensor C, ws;
  if (use_ws) {
    ws = torch::empty({(int64_t)splitm, (int64_t)N, (int64_t)Kw}, f32);
    C = torch::empty({(int64_t)N, (int64_t)Kw}, out_bf16 ? dz.options() : f32);
  } else {
    C = torch::empty({(int64_t)N, (int64_t)Kw}, f32);
  }
  const size_t shmem = (size_t)RING * SLOT_BYTES;  // 80 KiB
#define LAUNCH_TN(DBO, WSO)                                                                \
  launch_lds<gemm_tn_128_kernel<DBO, WSO>>(                                                \
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

torch::Tensor gemm_tn_128(torch::Tensor dz, torch::Tensor x, int64_t splitm, bool out_bf16) {
  return tn128_run(dz, x, nullptr, splitm, out_bf16);
}

std::vector<torch::Tensor> gemm_tn_128_db(torch::Tensor dz, torch::Tensor x, int64_t splitm,
                                          bool out_bf16) {
  // fused dW + bias-grad: {dW (N, Kw) fp32 or bf16, db (N) fp32}
  TORCH_CHECK(dz.is_cuda() && dz.dim() == 2);
  auto db = torch::zeros({dz.size(1)}, dz.options().dtype(torch::kFloat32));
  auto C = tn128_run(dz, x, db.data_ptr<float>(), splitm, out_bf16);
  return {C, db};
}
