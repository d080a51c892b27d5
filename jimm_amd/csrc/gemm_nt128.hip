// NT forward / dX GEMM for shapes off the 256 grid:
// Y[M,N] = epilogue(X[M,K] @ W[N,K]^T), 128x128 output tiles, ragged M, N and
// K, MFMA bf16 with fp32 accumulation.  The 8-phase kernel (gemm8p.hip) needs
// N % 256 == 0 and K % 64 == 0; this one takes any M >= 1, N % 8 == 0,
// K % 8 == 0 — the N / K domain of gemm_tn_128, so every weight whose dW runs
// in-house can run its forward and dX in-house too (ViT-S/Ti 384 / 192,
// so400m 1152 / 3456 / 4304).  Which shapes reach it is the rule of
// ops/hip_linear.py (_nt128_ok) and ops/block.py (_hip_gemms).
//
// Tile and waves: 256 threads, four waves laid out 2 (wm: rows) x 2 (wn:
// columns), each owning 64 x 64 = acc[4][4] of f32x4 on
// v_mfma_f32_16x16x32_bf16.  Workgroups walk ceil(M/128) * ceil(N/128) tiles
// through xcd_remap, n fastest.
//
// Staging unit: one K-half, the 32 k-columns [32u, 32u + 32) of X's 128 rows
// and of W's 128 rows.  Each operand's unit image is 8 KiB, 128 rows of 64
// bytes (4 chunks of 16 B):
//   byte(row, c) = row*64 + ((c ^ ((row >> 2) & 3)) << 4)
// filled by glds16 (lane-linear destination, 2 rounds of 4 KiB per operand,
// the inverse permutation on the per-lane SOURCE address: 4 glds per thread
// and unit) and read back as MFMA fragments with ds_read_b128: fragment row
// 16i + lo, chunk hi.  The 16 lanes of one hi are rows lo = 0..15: (row & 3)
// picks one of four 64-byte quarters of the 256-byte bank window and
// hi ^ ((row >> 2) & 3) one of its four 16-byte groups, so they hit 16
// distinct bank groups.
//
// Ragged M and N are OUTPUT dimensions and need no zero fill: a staging lane
// whose row lies beyond the edge reads row M-1 (N-1) instead — a valid
// address — and what it brings in lands only in accumulator rows / columns
// that the predicated epilogue never stores.
//
// Column mapping: image row j of the W unit holds W row
// n0 + (j & ~63) + 4*(j & 15) + ((j >> 4) & 3), clamped AFTER permuting (the
// 8-phase kernel's permutation, gemm8p.hip).  acc[mi][ni][r] is then row
// m0 + wm*64 + 16mi + 4hi + r, column n0 + wn*64 + 4lo + ni: a lane holds 4
// consecutive columns of a row and gemm_epilogue4 (mfma.h) makes one 8-byte
// access per stream for them, and one bias load per tile.  N % 8 == 0 puts a
// 4-column group wholly inside or wholly outside the matrix.
//
// Ring: a slot is 16 KiB (X image at +0, W image at +8 KiB), RING = 5 slots
// are 80 KiB, so TWO workgroups share a CU: one's barrier and fragment reads
// run under the other's MFMAs.  Unit u lives in slot u % RING.  One unit is
// ONE phase with one raw s_barrier:
//   P(u): 4 + 4 ds_read_b128 of slot(u); lgkmcnt(0); counted vmcnt; barrier
//         B(u); issue unit u+RING into slot(u); 16 MFMA under s_setprio(1)
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
//   So RING-1 units are in flight across barriers and no wave drains the
//   queue inside the loop.  The counted wait is exact because the loop holds
//   no other vector-memory instruction.
// Ragged K: K is the contraction, so the tail must add exact zeros.  The
// ring takes the K / 32 whole units; the K % 32 (8, 16 or 24) columns left
// are staged after the ring has drained (the last unit's wait is vmcnt(0) and
// B(last) has passed, so every slot is free and every read of it retired):
// guarded register loads (zero chunks at and beyond K, rows clamped as
// above), ds_write_b128 into slot 0, lgkmcnt(0), one barrier, the same walk.
// Nothing stale is multiplied by zero.
//
// Epilogue forms: bias (fp32 or bf16), erf-GELU / tanh-GELU / QuickGELU,
// residual, SAVE_NONE / SAVE_PRE / SAVE_GRAD, and the dX forms GRADM_MUL
// (saved fp16 derivative) and GRADM_ACT (saved bf16 pre-activation).  No
// dropout form (its Philox definition is tied to the unpermuted column
// mapping) and no e4m3 output.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <climits>

#include "mfma.h"

namespace {

typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int BM = 128, BN = 128;
constexpr int BKU = 32;            // k-columns per staging unit
constexpr int NTHREADS = 256;
constexpr int UNIT_BYTES = 8192;   // one operand's 128 x 32 bf16 unit image
constexpr int SLOT_BYTES = 2 * UNIT_BYTES;  // X image + W image
constexpr int RING = 5;            // ring slots (RING * 16 KiB of LDS)
constexpr int GLDS_PER_UNIT = 4;   // per thread: 2 X + 2 W

// fp32 arithmetic is not to be packed in pairs (v_pk_*_f32) in this file: the
// device pass compiles every function and lambda below without the feature
// (one setting for all of them, or the lambdas would not be inlined).
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

// unit-image byte offset of chunk c (0..3) of row 0..127
__device__ __forceinline__ int img_off(int row, int c) {
  return row * 64 + ((c ^ ((row >> 2) & 3)) << 4);
}

// W row (within the 128-row tile) that image row j holds (header)
__device__ __forceinline__ int perm_row(int j) {
  return (j & ~63) + 4 * (j & 15) + ((j >> 4) & 3);
}

template <int ACT, bool HAS_BIAS, bool HAS_RES, int SAVE, int GRADM>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_nt_128_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ W, const void* __restrict__ bias,
    int bias_bf16, const bf16* __restrict__ res, bf16* __restrict__ Y, bf16* __restrict__ Z,
    int M, int N, int K) {
  // ring slot s at s*16 KiB: X unit image at +0, W unit image at +8 KiB
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wave = tid / WAVE;
  const int lo = lane & 15, hi = lane >> 4;

  const int mt = (M + BM - 1) / BM, nt = (N + BN - 1) / BN;
  const int wg = xcd_remap(blockIdx.x, mt * nt);
  const int m0 = (wg / nt) * BM;
  const int n0 = (wg % nt) * BN;
  const int wm = wave >> 1;  // 0..1 (row sub-position)
  const int wn = wave & 1;   // 0..1 (column sub-position)

  const int nunit = K / BKU;       // ring units
  const int ktail = K - nunit * BKU;  // 0, 8, 16 or 24 columns left

  f32x4_t acc[4][4] = {};  // [mi][ni]

  // Ring staging for this thread: round j of an operand covers unit-image
  // bytes [j*4096 + tid*16]: image row j*64 + tid/4, chunk position tid & 3,
  // whose content is source chunk pos ^ ((row >> 2) & 3) of the (clamped,
  // for W permuted) source row.  The pointers walk 32 columns per unit.
  const bf16* px[2];
  const bf16* pw[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = j * 64 + (tid >> 2);
    const int c = (tid & 3) ^ ((row >> 2) & 3);
    int gm = m0 + row, gn = n0 + perm_row(row);
    gm = gm < M ? gm : M - 1;
    gn = gn < N ? gn : N - 1;
    px[j] = X + (int64_t)gm * K + c * 8;
    pw[j] = W + (int64_t)gn * K + c * 8;
  }
  const int ldst16 = tid * 16;
  auto issue_unit = [&](char* slot) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      glds16(px[j], slot + j * 4096 + ldst16);
      px[j] += BKU;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      glds16(pw[j], slot + UNIT_BYTES + j * 4096 + ldst16);
      pw[j] += BKU;
    }
  };

  // K-tail staging into slot 0: the columns [nunit*32, K) of both operands'
  // 128 rows, zeros from K on; 128 rows x 4 chunks per operand in 2 rounds.
  // It runs once, after the ring has drained (header).
  auto stage_reg_tail = [&]() {
    const int kt0 = nunit * BKU;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int g = r * NTHREADS + tid;
      const int row = g >> 2, c = g & 3;
      int gm = m0 + row, gn = n0 + perm_row(row);
      gm = gm < M ? gm : M - 1;
      gn = gn < N ? gn : N - 1;
      bf16x8_t a = bf16x8_t{}, b = bf16x8_t{};
      if (c * 8 < ktail) {
        a = *reinterpret_cast<const bf16x8_t*>(X + (int64_t)gm * K + kt0 + c * 8);
        b = *reinterpret_cast<const bf16x8_t*>(W + (int64_t)gn * K + kt0 + c * 8);
      }
      char* at = smem + img_off(row, c);
      *reinterpret_cast<bf16x8_t*>(at) = a;
      *reinterpret_cast<bf16x8_t*>(at + UNIT_BYTES) = b;
    }
  };

  // Per-lane fragment read offset: row 16i + lo of the wave's 64, chunk hi;
  // (row >> 2) & 3 == (lo >> 2) & 3 for every i, so fragment i lies i*1024
  // bytes further on.
  const int frag_a = img_off(wm * 64 + lo, hi);
  const int frag_b = UNIT_BYTES + img_off(wn * 64 + lo, hi);

  // One unit = one phase.  before_b runs ahead of the barrier, after_b right
  // behind it (the ring's wait / issue points; empty for the tail).
  auto consume_unit = [&](const char* slot, auto&& before_b,
                          auto&& after_b) __attribute__((always_inline)) {
    typedef const __attribute__((address_space(3))) char* lds_p;
    const lds_p ai = (lds_p)(const void*)(slot + frag_a);
    const lds_p bi = (lds_p)(const void*)(slot + frag_b);
    bf16x8_t xa[4], wb[4];
    asm volatile(
        "ds_read_b128 %0, %8 offset:0\n\t"
        "ds_read_b128 %1, %8 offset:1024\n\t"
        "ds_read_b128 %2, %8 offset:2048\n\t"
        "ds_read_b128 %3, %8 offset:3072\n\t"
        "ds_read_b128 %4, %9 offset:0\n\t"
        "ds_read_b128 %5, %9 offset:1024\n\t"
        "ds_read_b128 %6, %9 offset:2048\n\t"
        "ds_read_b128 %7, %9 offset:3072\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(xa[0]), "=&v"(xa[1]), "=&v"(xa[2]), "=&v"(xa[3]), "=&v"(wb[0]), "=&v"(wb[1]),
          "=&v"(wb[2]), "=&v"(wb[3])
        : "v"(ai), "v"(bi)
        : "memory");
    __builtin_amdgcn_sched_barrier(0);
    before_b();
    raw_barrier();
    after_b();
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = MFMA16(xa[mi], wb[ni], acc[mi][ni]);
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
  if (ktail) {
    // the ring is drained and every slot is free (see header)
    stage_reg_tail();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    raw_barrier();
    consume_unit(smem, [] {}, [] {});
  }

  // Epilogue: acc[mi][.][r] -> row m0 + wm*64 + 16mi + 4hi + r, columns
  // n .. n+3 with n = n0 + wn*64 + 4lo, inside the matrix only.
  const int n = n0 + wn * 64 + 4 * lo;
  if (n >= N) return;
  float bv[4] = {};
  if (HAS_BIAS) load_bias4(bias, n, bias_bf16, bv);
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm * 64 + 16 * mi + hi * 4 + r;
      if (m >= M) continue;
      const float v4[4] = {acc[mi][0][r], acc[mi][1][r], acc[mi][2][r], acc[mi][3][r]};
      gemm_epilogue4<ACT, HAS_BIAS, HAS_RES, SAVE, GRADM>(v4, m, n, N, bv, res, Y, Z);
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

bool aligned_to(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// One launch: 80 KiB of LDS, one workgroup per 128 x 128 output tile.
template <auto Kernel>
void launch_nt128(const torch::Tensor& x, const torch::Tensor& w, const void* biasp,
                  int bias_bf16, const void* resp, torch::Tensor& y, void* zp) {
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  // the 4-wide epilogue's vector accesses (N % 8 == 0 keeps every row and
  // column offset a multiple of the access; the bases are checked here)
  TORCH_CHECK(aligned_to(y.data_ptr(), 8) && aligned_to(resp, 8) && aligned_to(zp, 8),
              "gemm_nt_128: y, residual / z / g and the saved tensor must be 8-byte aligned");
  TORCH_CHECK(aligned_to(biasp, bias_bf16 ? 8 : 16),
              "gemm_nt_128: a bf16 bias must be 8-byte, an fp32 bias 16-byte aligned");
  constexpr size_t shmem = (size_t)RING * SLOT_BYTES;  // 80 KiB
  const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  launch_lds<Kernel>(dim3(tiles), dim3(NTHREADS), shmem, shmem, at::hip::getCurrentHIPStream(),
                     reinterpret_cast<const bf16*>(x.data_ptr()),
                     reinterpret_cast<const bf16*>(w.data_ptr()), biasp, bias_bf16,
                     static_cast<const bf16*>(resp), reinterpret_cast<bf16*>(y.data_ptr()),
                     static_cast<bf16*>(zp), M, N, K);
}

}  // namespace

bool gemm_nt_128_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0 && M <= INT_MAX - BM &&
         N <= INT_MAX - BN && K <= INT_MAX &&
         ((M + BM - 1) / BM) * ((N + BN - 1) / BN) <= INT_MAX;
}

namespace {

// Checks shared by the three entry points, all ahead of any launch: x (M, K)
// and w (N, K) contiguous 16-byte-aligned bf16 inside the kernel's domain.
void check_nt128(const char* op, const torch::Tensor& x, const torch::Tensor& w) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && x.dim() == 2 && w.dim() == 2, op,
              ": x (M, K) and w (N, K) must be 2-d CUDA tensors");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && w.scalar_type() == torch::kBFloat16, op,
              ": operands must be bf16");
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous(), op, ": operands must be contiguous");
  TORCH_CHECK(w.size(1) == x.size(1) && gemm_nt_128_supported(x.size(0), w.size(0), x.size(1)),
              op, ": needs M >= 1 and N, K multiples of 8, got x ", x.sizes(), " w ", w.sizes());
  TORCH_CHECK(aligned_to(x.data_ptr(), 16) && aligned_to(w.data_ptr(), 16), op,
              ": operands must be 16-byte aligned");
}

}  // namespace

// y = act(x @ w^T + bias) [+ residual] -> {y, z}: z per `save` — "none"
// (undefined = None in Python), "pre" (the bf16 pre-activation) or "grad" (the
// fp16 activation derivative; needs an activation). bias: fp32 or bf16, read
// as it is; any other dtype goes through fp32.
std::vector<torch::Tensor> gemm_nt_128(torch::Tensor x, torch::Tensor w,
                                       c10::optional<torch::Tensor> bias, std::string act,
                                       c10::optional<torch::Tensor> residual, std::string save) {
  check_nt128("gemm_nt_128", x, w);
  const int64_t M = x.size(0), N = w.size(0);
  const int save_c = save == "none" ? SAVE_NONE : save == "pre" ? SAVE_PRE : save == "grad" ? SAVE_GRAD : -1;
  TORCH_CHECK(save_c >= 0, "gemm_nt_128: save must be none, pre or grad, got ", save);
  const int act_i = act_code(act);
  TORCH_CHECK(save_c != SAVE_GRAD || act_i != ACT_NONE,
              "saving the activation derivative needs an activation");
  if (residual)
    TORCH_CHECK(residual->is_cuda() && residual->is_contiguous() &&
                    residual->scalar_type() == torch::kBFloat16 && residual->numel() == M * N,
                "gemm_nt_128: the residual must be a contiguous bf16 (M, N)");
  c10::optional<torch::Tensor> b;
  if (bias) {
    TORCH_CHECK(bias->is_cuda() && bias->numel() == N, "gemm_nt_128: bias must hold N values");
    b = bias->contiguous();
    if (b->scalar_type() != torch::kBFloat16 && b->scalar_type() != torch::kFloat32)
      b = b->to(torch::kFloat32);
  }
  auto y = torch::empty({M, N}, x.options());
  torch::Tensor z;
  if (save_c == SAVE_PRE) z = torch::empty({M, N}, x.options());
  if (save_c == SAVE_GRAD) z = torch::empty({M, N}, x.options().dtype(torch::kFloat16));
  const void* biasp = b ? b->data_ptr() : nullptr;
  const int bias_bf16 = b && b->scalar_type() == torch::kBFloat16;
  const void* resp = residual ? residual->data_ptr() : nullptr;
  void* zp = z.defined() ? z.data_ptr() : nullptr;
  with_act(act_i, [&](auto act_c) {
    with_save(save_c, [&](auto sv) {
      with_flags(
          [&](auto hb, auto hr) {
            constexpr int A = decltype(act_c)::value, S = decltype(sv)::value;
            if constexpr (S != SAVE_GRAD || A != ACT_NONE)
              launch_nt128<gemm_nt_128_kernel<A, decltype(hb)::value, decltype(hr)::value, S,
                                              GRADM_NONE>>(x, w, biasp, bias_bf16, resp, y, zp);
          },
          bias.has_value(), residual.has_value());
    });
  });
  return {y, z};
}

// dz = (dy @ wt^T) * g on a pre-transposed wt (in_f, out_f), g the fp16
// activation derivative a SAVE_GRAD forward stored.
torch::Tensor gemm_nt_128_gradmul(torch::Tensor dy, torch::Tensor wt, torch::Tensor g) {
  check_nt128("gemm_nt_128_gradmul", dy, wt);
  TORCH_CHECK(g.is_cuda() && g.is_contiguous() && g.scalar_type() == torch::kFloat16 &&
                  g.dim() == 2 && g.size(0) == dy.size(0) && g.size(1) == wt.size(0),
              "gemm_nt_128_gradmul: g must be a contiguous fp16 (M, N)");
  auto y = torch::empty({dy.size(0), wt.size(0)}, dy.options());
  launch_nt128<gemm_nt_128_kernel<ACT_NONE, false, true, SAVE_NONE, GRADM_MUL>>(
      dy, wt, nullptr, 0, g.data_ptr(), y, nullptr);
  return y;
}

// dz = (dy @ wt^T) * act'(z), z the saved bf16 pre-activation.
torch::Tensor gemm_nt_128_gradact(torch::Tensor dy, torch::Tensor wt, torch::Tensor z,
                                  std::string act) {
  check_nt128("gemm_nt_128_gradact", dy, wt);
  TORCH_CHECK(z.is_cuda() && z.is_contiguous() && z.scalar_type() == torch::kBFloat16 &&
                  z.dim() == 2 && z.size(0) == dy.size(0) && z.size(1) == wt.size(0),
              "gemm_nt_128_gradact: z must be a contiguous bf16 (M, N)");
  const int act_i = act_code(act);
  TORCH_CHECK(act_i != ACT_NONE, "gradact needs an activation, got ", act);
  auto y = torch::empty({dy.size(0), wt.size(0)}, dy.options());
  with_act(act_i, [&](auto act_c) {
    constexpr int A = decltype(act_c)::value;
    if constexpr (A != ACT_NONE)
      launch_nt128<gemm_nt_128_kernel<A, false, true, SAVE_NONE, GRADM_ACT>>(
          dy, wt, nullptr, 0, z.data_ptr(), y, nullptr);
  });
  return y;
}
