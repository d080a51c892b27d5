// e4m3 256x256-tile MFMA GEMM with fused epilogue:
//   Y[M,N] (bf16) = epilogue( (sa*sb) * A8[M,K] @ B8[N,K]^T )
// A8, B8 row-major OCP e4m3 bytes (what layernorm_fwd_fp8, bias_act_fwd_fp8 and
// the gradact GEMM emit); sa, sb fp32 DEVICE scalars read once per workgroup
// (no host sync, graph-capturable); fp32 accumulation; sa*sb multiplies the
// accumulator before the bias.
//
// The K loop is built on v_mfma_f32_16x16x128_f8f6f4 (format selectors at
// their fp8 default, no block scales): one instruction contracts a whole
// 128-byte image row, so a K-tile (BK = 128 elements = one 128-byte row per
// operand row) is ONE MFMA deep. There are no K-halves to walk; the walk is
// over the row-halves alone:
//
// Phase walk, two phases per K-tile (pr = row-half):  p0 = pr0   p1 = pr1
// Wave (wm,wn) of 8 computes rows [pr*128+wm*64,+64) x cols [wn*64,+64) at the
// tile's full K depth per phase: p0 reads 4 A-fragments of A-half 0 and the 4
// B-fragments of the tile, p1 reads 4 A-fragments of A-half 1 and REUSES the
// B-fragments in registers. A fragment is 32 bytes per lane = two
// ds_read_b128, so a K-tile costs a wave 24 ds_read_b128 for 32 MFMAs - each
// byte of the wave's 16 KiB A + 8 KiB B strips leaves LDS exactly once.
//
// Chunk mapping. Lane (hi = lane>>4, lo = lane&15) supplies the instruction
// with 32 K-values of fragment row lo; which 32 of the row's 128 is free as
// long as A and B agree (a contraction does not care about the order of K).
// A lane takes the 16-byte chunks {hi, 4 + hi} of its row: read j (j = 0, 1)
// of a fragment is lane (hi, lo) -> row base + lo, chunk 4j + hi, swizzled to
// byte row*128 + ((4j + hi) ^ (row & 7))*16. Bank-conflict freedom: in one
// read the 8 lanes lo..lo+7 of a hi hold 8 consecutive rows, so row & 7 runs
// over all 8 values and the XOR sends the one chunk index to 8 DIFFERENT
// 16-byte slots; rows alternate between the two 128-byte halves of the
// 256-byte bank line, and different hi differ in the chunk index, i.e. in the
// slot of every row. This is, address for address, the ds_read_b128 the bf16
// 8-phase kernel issues for its K-half j (gemm8p.hip: row lo, chunk 4kh + hi),
// whose measured bank-conflict count is zero. The alternative {2hi, 2hi + 1}
// would give a lane one contiguous 32 bytes but make read j's chunk index
// 2hi + j, which is the same access set per instruction pair and no better;
// {hi, 4 + hi} makes the second address the first XOR 64 (one offset register
// per fragment).
//
// LDS: 9 half-images of 16 KiB (128 rows x 128 B) = 144 KiB of the 160 KiB:
//   A0[2] A1[2]  (tile parity)   B1[2] (tile parity)   B0[3] (tile mod 3)
// image swizzle byte(row, c16) = row*128 + (c16 ^ (row&7))*16; glds16 writes
// lane-linear, the inverse permutation is on the per-lane SOURCE address. The
// W operand is staged with the PERM row permutation of gemm8p.hip (image row
// j of a 64-row group takes W row 4*(j&15) + ((j>>4)&3)), so a lane's 4
// accumulator columns are 4 consecutive columns and gemm_epilogue4 applies.
//
// Staging (2 half-images = 4 glds16 per lane and phase), phase f = 2t + pr:
//   p0 of tile t -> A0(t+1), B1(t+1)      p1 of tile t -> A1(t+1), B0(t+2)
// A phase is { ds_reads; stage; s_waitcnt vmcnt(n); s_barrier; MFMAs }.
//
// Slot reuse. A wave's reads of phase f complete before its MFMAs of phase f
// (compiler lgkmcnt), hence before it arrives at barrier f+1; a stage of
// phase g is issued after barrier g-1. A slot last read in phase f may be
// overwritten from phase f+2 on:
//   A0(t+1), B1(t+1) staged in 2t   over A0(t-1), B1(t-1), last read 2t-2
//   A1(t+1)          staged in 2t+1 over A1(t-1),          last read 2t-1
//   B0(t+2)          staged in 2t+1 over B0(t-1),          last read 2t-2
// (B0 runs a tile further ahead so that every half-image has a full phase
// between its issue and the wait that certifies it; with 2 slots it would
// land on B0(t), read in 2t: one barrier, a DMA-vs-pending-read race.)
//
// Wait counts (issue order ... A1(t) B0(t+1) | A0(t+1) B1(t+1) | A1(t+1)
// B0(t+2) | ..., 2 glds each; reads of phase f+1 follow barrier f, which
// follows every wave's wait of phase f):
//   p0 of t must certify A1(t) (read in p1 of t). Younger: B0(t+1) and this
//     phase's A0(t+1), B1(t+1) -> vmcnt(6); last tile: none exist, vmcnt(0).
//   p1 of t must certify A0(t+1), B1(t+1) (issued in p0) and B0(t+1) (older).
//     Younger: this phase's A1(t+1) [t+1 < nk] and B0(t+2) [t+2 < nk]
//     -> vmcnt(4), vmcnt(2) on the last but one tile, vmcnt(0) on the last.
//   Prologue issues B0(0) A0(0) B1(0) A1(0) B0(1); vmcnt(4) certifies the
//     first three for p0 of tile 0 and leaves A1(0), B0(1) to p0's vmcnt(6).
// K >= 256 (two tiles) keeps B0(1) unconditional.
//
// Epilogue: gemm_epilogue4 (mfma.h) on acc * (sa*sb): bias fp32 or bf16,
// ACT_*, residual, SAVE_PRE, and FP8O (e4m3 copy of Y under a delayed scale,
// amax by wave reduction + atomicMax, as gemm_nt_8p_kernel). The accumulator
// layout is that of the bf16 16x16x32 instruction: lane (hi, lo) holds rows
// 4*hi + r, column lo. M may be ragged (MGUARD clamps staged rows, predicates
// stores); N % 256 == 0, K % 128 == 0, K >= 256 (gemm_f8_supported).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "mfma.h"

namespace {

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned char u8;

constexpr int BM = 256, BN = 256, BK = 128;  // BK in elements = bytes
constexpr int NTHREADS = 512;
constexpr int HALF_BYTES = 128 * BK;  // 16 KiB per half-image
constexpr int NHALVES = 9;

// fp32 arithmetic is not to be packed in pairs (v_pk_*_f32) in this file: the
// device pass compiles every function and lambda below without the feature
// (one setting for all of them, or the lambdas would not be inlined).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define MFMA_F8(A, B, C) \
  __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A, B, C, 0, 0, 0, 0, 0, 0)

// Per-lane glds source of one half-image: 512 threads x 16 B x 2 rounds;
// round r, thread tid covers image byte off = r*8192 + tid*16. Row and chunk
// are fixed per lane, the K loop adds kt*128 bytes. PERM: gemm8p.hip.
template <bool MGUARD, bool PERM>
__device__ __forceinline__ const u8* stage_base_f8(const u8* __restrict__ gsrc, int64_t ldg,
                                                   int row0, int rows_total, int round,
                                                   int tid) {
  const int off = round * 8192 + tid * 16;
  const int row = off >> 7;
  const int chunk = ((off >> 4) & 7) ^ (row & 7);
  int grow = row0 + (PERM ? (row & ~63) + 4 * (row & 15) + ((row >> 4) & 3) : row);
  if (MGUARD) grow = grow < rows_total ? grow : rows_total - 1;
  return gsrc + (int64_t)grow * ldg + chunk * 16;
}

// The 32-byte fragment of a lane: chunks {hi, 4 + hi} of its row; off is the
// swizzled byte of chunk hi, chunk 4 + hi lies at off ^ 64.
__device__ __forceinline__ i32x8_t lds_frag_f8(const char* base, int off) {
  const i32x4_t c0 = *reinterpret_cast<const i32x4_t*>(base + off);
  const i32x4_t c1 = *reinterpret_cast<const i32x4_t*>(base + (off ^ 64));
  return __builtin_shufflevector(c0, c1, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int ACT, bool HAS_BIAS, bool HAS_RES, int SAVE, bool MGUARD, bool FP8O>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_nt_f8_kernel(
    const u8* __restrict__ X, const u8* __restrict__ W, const float* __restrict__ sa,
    const float* __restrict__ sb, const void* __restrict__ bias, int bias_bf16,
    const bf16* __restrict__ res, bf16* __restrict__ Y, bf16* __restrict__ Z, int M, int N,
    int K, u8* __restrict__ Y8, const float* __restrict__ scale8,
    unsigned int* __restrict__ amax_bits) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // half-images: A[buf 0..1][half 0..1] | B1[buf 0..1] | B0[slot 0..2]
  auto As = [&](int buf, int h) { return smem + (buf * 2 + h) * HALF_BYTES; };
  auto B1s = [&](int buf) { return smem + (4 + buf) * HALF_BYTES; };
  auto B0s = [&](int slot) { return smem + (6 + slot) * HALF_BYTES; };

  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wave = tid / WAVE;
  const int lo = lane & 15, hi = lane >> 4;

  const int mt = MGUARD ? (M + BM - 1) / BM : M / BM;
  const int nt = N / BN;
  const int wg = xcd_remap(blockIdx.x, mt * nt);
  const int m0 = (wg / nt) * BM;
  const int n0 = (wg % nt) * BN;
  const int wm = (wave >> 2);  // 0..1
  const int wn = (wave & 3);   // 0..3

  f32x4_t acc[2][4][4] = {};  // [pr][mi][ni]

  const int nk = K / BK;  // >= 2
  const u8* asrc[2][2];   // [half][round]
  const u8* bsrc[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      asrc[h][r] = stage_base_f8<MGUARD, false>(X, K, m0 + h * 128, M, r, tid);
      bsrc[h][r] = stage_base_f8<false, true>(W + (int64_t)n0 * K, K, h * 128, N, r, tid);
    }
  const int ldst = tid * 16;
  auto stage2 = [&](const u8* r0, const u8* r1, int kt, char* img) {
    glds16(reinterpret_cast<const bf16*>(r0 + (int64_t)kt * BK), img + ldst);
    glds16(reinterpret_cast<const bf16*>(r1 + (int64_t)kt * BK), img + 8192 + ldst);
  };
  auto stageA = [&](int h, int kt, char* img) { stage2(asrc[h][0], asrc[h][1], kt, img); };
  auto stageB = [&](int h, int kt, char* img) { stage2(bsrc[h][0], bsrc[h][1], kt, img); };

  // Per-lane fragment offsets (chunk hi; chunk 4 + hi is the offset ^ 64).
  // The wave's 64 columns live in B-half (wn >> 1) at rows (wn&1)*64 + 16ni + lo.
  int offA[4], offB[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ra = wm * 64 + 16 * i + lo, rb = (wn & 1) * 64 + 16 * i + lo;
    offA[i] = (ra << 7) + ((hi ^ (ra & 7)) << 4);
    offB[i] = (rb << 7) + ((hi ^ (rb & 7)) << 4);
  }
  const int bh = wn >> 1;

  // Prologue: B0(0) A0(0) B1(0) A1(0) B0(1); certify the first three.
  stageB(0, 0, B0s(0));
  stageA(0, 0, As(0, 0));
  stageB(1, 0, B1s(0));
  stageA(1, 0, As(0, 1));
  stageB(0, 1, B0s(1));
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  raw_barrier();

  int s0 = 0, s2 = 2;  // B0 slots of tiles t and t+2
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    const char* bi = bh ? B1s(buf) : B0s(s0);
    const bool more = t + 1 < nk, more2 = t + 2 < nk;

    // ---- p0: A-half 0 + the tile's B fragments; stage A0(t+1), B1(t+1) ----
    i32x8_t xa[4], wb[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) xa[mi] = lds_frag_f8(As(buf, 0), offA[mi]);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) wb[ni] = lds_frag_f8(bi, offB[ni]);
    if (more) {
      stageA(0, t + 1, As(buf ^ 1, 0));
      stageB(1, t + 1, B1s(buf ^ 1));
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    raw_barrier();
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[0][mi][ni] = MFMA_F8(xa[mi], wb[ni], acc[0][mi][ni]);
    __builtin_amdgcn_s_setprio(0);

    // ---- p1: A-half 1, B fragments reused; stage A1(t+1), B0(t+2) ----
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) xa[mi] = lds_frag_f8(As(buf, 1), offA[mi]);
    if (more2) {
      stageA(1, t + 1, As(buf ^ 1, 1));
      stageB(0, t + 2, B0s(s2));
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else if (more) {
      stageA(1, t + 1, As(buf ^ 1, 1));
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    raw_barrier();
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[1][mi][ni] = MFMA_F8(xa[mi], wb[ni], acc[1][mi][ni]);
    __builtin_amdgcn_s_setprio(0);

    s0 = s0 + 1 == 3 ? 0 : s0 + 1;
    s2 = s2 + 1 == 3 ? 0 : s2 + 1;
  }

  // Epilogue: acc[pr][mi][ni][r] -> row m0 + pr*128 + wm*64 + 16mi + hi*4 + r,
  // col n0 + wn*64 + 4lo + ni.
  const float sab = sa[0] * sb[0];
  float rs8 = 1.f, tmax = 0.f;
  if (FP8O) rs8 = fast_rcpf(scale8[0]);
  const int n = n0 + wn * 64 + 4 * lo;
  float bv[4] = {};
  if (HAS_BIAS) load_bias4(bias, n, bias_bf16, bv);
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + pr * 128 + wm * 64 + 16 * mi + hi * 4 + r;
        if (MGUARD && m >= M) continue;
        const float v4[4] = {acc[pr][mi][0][r] * sab, acc[pr][mi][1][r] * sab,
                             acc[pr][mi][2][r] * sab, acc[pr][mi][3][r] * sab};
        gemm_epilogue4<ACT, HAS_BIAS, HAS_RES, SAVE, GRADM_NONE, FP8O>(v4, m, n, N, bv, res, Y,
                                                                       Z, Y8, rs8, &tmax);
      }
    }
  }
  if (FP8O) {
    tmax = wave_reduce_max(tmax);
    // builtins, not the header's atomicMax / __float_as_uint: those are plain
    // inline functions compiled with the feature and would become calls here
    if (lane == 0)
      __hip_atomic_fetch_max(amax_bits, __builtin_bit_cast(unsigned int, tmax), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

bool aligned_to(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace

bool gemm_f8_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && (N % BN == 0) && (K % BK == 0) && K >= 2 * BK;
}

// y = act((sa*sb) * a8 @ b8^T + bias) [+ res] on e4m3 bytes -> {y, z, y8}:
// z the bf16 pre-activation (save_pre), y8 the e4m3 copy of y under
// scale_out with its amax combined into amax_out (both or neither); absent
// ones are undefined tensors (None in Python). Outside gemm_f8_supported or
// with a misaligned base this raises before any launch; there is no other
// route inside the extension.
// Instantiated forms: without an activation any of bias / residual; with an
// activation always SAVE_PRE; the e4m3 emission with activation + bias and no
// residual (the MLP's fc1).
std::vector<torch::Tensor> linear_fwd_f8(torch::Tensor a8, torch::Tensor sa, torch::Tensor b8,
                                         torch::Tensor sb, c10::optional<torch::Tensor> bias,
                                         std::string act, c10::optional<torch::Tensor> res,
                                         bool save_pre, c10::optional<torch::Tensor> scale_out,
                                         c10::optional<torch::Tensor> amax_out) {
  auto is_byte = [](const torch::Tensor& t) {
    return t.scalar_type() == torch::kUInt8 || t.scalar_type() == torch::kFloat8_e4m3fn;
  };
  auto is_scalar = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.device() == a8.device() && t.scalar_type() == torch::kFloat32 &&
           t.numel() == 1;
  };
  TORCH_CHECK(a8.is_cuda() && b8.is_cuda() && a8.device() == b8.device(),
              "linear_fwd_f8: operands must be on one GPU");
  TORCH_CHECK(is_byte(a8) && is_byte(b8), "linear_fwd_f8: operands must be e4m3 bytes");
  TORCH_CHECK(a8.dim() == 2 && b8.dim() == 2 && a8.is_contiguous() && b8.is_contiguous());
  TORCH_CHECK(is_scalar(sa) && is_scalar(sb), "linear_fwd_f8: scales are fp32 device scalars");
  const int64_t M = a8.size(0), K = a8.size(1), N = b8.size(0);
  TORCH_CHECK(b8.size(1) == K, "linear_fwd_f8: a8 is (M, K), b8 is (N, K)");
  TORCH_CHECK(gemm_f8_supported(M, N, K), "linear_fwd_f8 needs N % 256 == 0, K % 128 == 0 and "
              "K >= 256, got M=", M, " N=", N, " K=", K);
  TORCH_CHECK(M < (int64_t(1) << 31) - BM && N < (int64_t(1) << 31) && K < (int64_t(1) << 31),
              "linear_fwd_f8: a dimension does not fit the kernel's 32-bit indices");
  TORCH_CHECK(aligned_to(a8.data_ptr(), 16) && aligned_to(b8.data_ptr(), 16),
              "linear_fwd_f8: the e4m3 operands must be 16-byte aligned");
  const int actc = act_code(act);
  const bool fp8o = scale_out.has_value();
  TORCH_CHECK(fp8o == amax_out.has_value(), "linear_fwd_f8: scale_out and amax_out go together");
  TORCH_CHECK(save_pre == (actc != ACT_NONE),
              "linear_fwd_f8: the pre-activation is saved exactly when there is an activation");
  TORCH_CHECK(!fp8o || (actc != ACT_NONE && bias && !res),
              "linear_fwd_f8: the e4m3 emission is built for activation + bias, no residual");
  if (fp8o) TORCH_CHECK(is_scalar(*scale_out) && is_scalar(*amax_out));

  const auto opt = a8.options().dtype(torch::kBFloat16);
  c10::optional<torch::Tensor> b;
  if (bias) {
    TORCH_CHECK(bias->numel() == N && bias->device() == a8.device());
    b = bias->contiguous();
    if (b->scalar_type() != torch::kBFloat16 && b->scalar_type() != torch::kFloat32)
      b = b->to(torch::kFloat32);
  }
  if (res)
    TORCH_CHECK(res->is_cuda() && res->is_contiguous() &&
                res->scalar_type() == torch::kBFloat16 && res->numel() == M * N);
  auto y = torch::empty({M, N}, opt);
  torch::Tensor z, y8;
  if (save_pre) z = torch::empty({M, N}, opt);
  if (fp8o) y8 = torch::empty({M, N}, opt.dtype(torch::kUInt8));

  const void* biasp = b ? b->data_ptr() : nullptr;
  const int bias_bf16 = b && b->scalar_type() == torch::kBFloat16;
  const bf16* resp = res ? reinterpret_cast<const bf16*>(res->data_ptr()) : nullptr;
  bf16* zp = save_pre ? bf16_ptr(z) : nullptr;
  u8* y8p = fp8o ? y8.data_ptr<u8>() : nullptr;
  const float* so = fp8o ? scale_out->data_ptr<float>() : nullptr;
  unsigned int* am = fp8o ? reinterpret_cast<unsigned int*>(amax_out->data_ptr()) : nullptr;
  // gemm_epilogue4's vector accesses (N % 256 == 0 keeps the offsets aligned)
  TORCH_CHECK(aligned_to(y.data_ptr(), 8) && aligned_to(resp, 8) && aligned_to(zp, 8) &&
                  aligned_to(y8p, 4) && aligned_to(biasp, bias_bf16 ? 8 : 16),
              "linear_fwd_f8: y / residual / z need 8-byte, the e4m3 output 4-byte, a bf16 bias "
              "8-byte and an fp32 bias 16-byte alignment");

  constexpr size_t shmem = NHALVES * HALF_BYTES;
  const int mt = (M + BM - 1) / BM;
  auto launch = [&](auto kernel_c) {
    launch_lds<decltype(kernel_c)::value>(
        dim3(mt * (N / BN)), dim3(NTHREADS), shmem, shmem, at::hip::getCurrentHIPStream(),
        reinterpret_cast<const u8*>(a8.data_ptr()), reinterpret_cast<const u8*>(b8.data_ptr()),
        sa.data_ptr<float>(), sb.data_ptr<float>(), biasp, bias_bf16, resp, bf16_ptr(y), zp,
        (int)M, (int)N, (int)K, y8p, so, am);
  };
  with_act(actc, [&](auto act_c) {
    with_flags(
        [&](auto hb, auto hr, auto mg, auto f8) {
          constexpr int A = decltype(act_c)::value;
          constexpr bool HB = decltype(hb)::value, HR = decltype(hr)::value;
          constexpr bool MG = decltype(mg)::value, F8 = decltype(f8)::value;
          constexpr int S = A != ACT_NONE ? SAVE_PRE : SAVE_NONE;
          if constexpr (!F8 || (A != ACT_NONE && HB && !HR))
            launch(std::integral_constant<decltype(&gemm_nt_f8_kernel<A, HB, HR, S, MG, F8>),
                                          &gemm_nt_f8_kernel<A, HB, HR, S, MG, F8>>{});
        },
        bias.has_value(), res.has_value(), (M % BM) != 0, fp8o);
  });
  return {y, z, y8};
}
