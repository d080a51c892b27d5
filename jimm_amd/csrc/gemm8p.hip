// K4/K6/K7/K8 — 8-phase 256x256-tile MFMA bf16 GEMM with fused epilogue.
//
// Deep-pipelined 256-square structure after the CDNA4 guide's 8-phase
// template (cdna_hip_programming.md §5): four sub-phases per K-tile, ONE raw
// s_barrier per phase (a wave's next-phase fragment reads overlap another
// wave's MFMA cluster), counted s_waitcnt vmcnt (never 0 in the main loop)
// so staged half-tiles stay in flight ACROSS barriers, s_setprio(1) around
// each 16-MFMA cluster (T5).
//
// Phase walk (kh = K-half of the 64-deep K-tile, pr = row-half):
//   p0=(kh0,pr0)  p1=(kh0,pr1)  p2=(kh1,pr0)  p3=(kh1,pr1)
// Wave (wm,wn) computes strip rows [pr*128+wm*64,+64) x cols [wn*64,+64) at
// K-depth 32 per phase: 4 A-frags + 4 B-frags ds_read_b128, 16 MFMA.  The
// B-fragments of a kh are REUSED in registers across the pr pair, so a
// K-tile costs 24 fragment reads per wave — the information-theoretic
// minimum (16 KiB A + 8 KiB B at 1 KiB per b128) — where a (row,col)
// quadrant walk costs 48.
//
// Staging (one half-image per phase; 2 glds per wave):
//   p0 -> B-half0(t+1)   p1 -> B-half1(t+1)   p2 -> A-half0(t+1)
//   p3 -> A-half1(t+1)
// A has 2x2 buffer slots (tile parity); B-half slots cycle mod 3 because B
// is read in EVERY phase (a 2-slot B would be overwritten one barrier after
// its last read — a DMA-vs-pending-ds_read race).  All slot-reuse gaps are
// >= 2 barriers; a wave's reads complete (hipcc lgkmcnt) before its own
// MFMA, hence before its next barrier arrival.  LDS = 4x16 KiB (A) +
// 6x16 KiB (B) = 160 KiB (the full CU LDS; occupancy 1 block/CU, 2
// waves/SIMD — the template's regime).
//
// Certification (reads at phase f follow the barrier at f-1, which follows
// every wave's counted vmcnt): vmcnt allowances {p0:2, p1:4, p2:4, p3:2}
// keep 1-2 half-tiles in flight and cover each half's stage->first-read lag
// (A0 staged t.p2 first read t+1.p0; A1 t.p3 -> t+1.p1; B t.p0/p1 ->
// t+1.p0).  The last tile's p0 drains with vmcnt(0) (its stages were the
// newest and the stream has ended).
//
// LDS image swizzle: byte(row, c16) = row*128 + (c16 ^ (row&7))*16 —
// verified conflict-free for this read pattern (SQ_LDS_BANK_CONFLICT = 0,
// profiles/r02: the ds_read_b128 16-lane groups mix chunk indices, so the
// row-XOR spreads them over all 16 slots).  glds writes lane-linear; the
// inverse permutation goes on the per-lane SOURCE address (§5.4 rule 21).
//
// Column mapping. In the MFMA accumulator layout a lane owns fragment column
// lo of each of its 4 B-fragments, i.e. columns 16*ni + lo of its wave's 64
// when image row j of a B half-image holds W row j: four columns 16 apart,
// every epilogue access 2 bytes wide. The non-dropout kernels (PERM = !DROP)
// instead stage W row 4*(j & 15) + ((j >> 4) & 3) of each 64-row group into
// image row j. Only the per-lane glds SOURCE row changes (stage_base): the
// image, its swizzle, offB / frag_off, every ds_read, wait and barrier of the
// K loop are what they were, and acc[pr][mi][ni][r] is now column 4*lo + ni —
// the same sum of the same products in the same order, so the same
// accumulator bits (what the epilogue makes of them: gemm_epilogue4, mfma.h).
// A lane's 4 values of a row are 4 consecutive columns, and gemm_epilogue4
// (mfma.h) makes one access per stream for them: 8 bytes of Y, Z / g,
// residual or saved z / g, 4 bytes of e4m3, and the 4 bias values in one
// 16-byte (fp32) or 8-byte (bf16) load per tile. 16 lanes cover 128
// contiguous bytes of a row.
// The DROP kernels keep the unpermuted mapping and the per-element epilogue:
// the dropout definition (docs/kernels.md) gives one Philox call to columns
// {c, c+16, c+32, c+48}, exactly the 4 columns a lane owns there; with 4
// consecutive columns a lane would make four calls and use one word of each.
//
// Epilogue fuses bias (fp32 or bf16, a lane's 4 values loaded once) +
// gelu/gelu_tanh/quickgelu (+residual) and saves nothing, the bf16
// pre-activation or the fp16 activation derivative (SAVE_*, mfma.h); the dX
// variants multiply by act'(z) recomputed from a saved z (GRADM_ACT) or by a
// saved fp16 derivative (GRADM_MUL: one load, convert and multiply per
// element, no activation code). DROP fuses counter-based dropout (common.h)
// into the two forward forms the MLP has: a lane's 16 elements of a fragment
// are the 4 words x 2 halves of two Philox calls, made in the epilogue loops.
// M may be ragged (MGUARD clamps staging rows and predicates stores);
// N%256==0, K%64==0, K>=128 required (gemm8p_supported). The 8-byte accesses
// need 8-byte aligned y / residual / z / g and bf16 bias, a 16-byte aligned
// fp32 bias and a 4-byte aligned e4m3 output; N%256==0 keeps every row and
// column offset aligned, the base pointers are checked in launch_8p.

#include <torch/extension.h>
#include <hip/hip_fp8.h>
#include <ATen/hip/HIPContext.h>

#include "mfma.h"

namespace {

typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int BM = 256, BN = 256, BK = 64;
constexpr int NTHREADS = 512;
constexpr int HALF_BYTES = 128 * BK * 2;  // 16 KiB per half-image

// Per-lane glds source base for one half-image (row/chunk fixed per lane;
// only the K offset advances — the K-loop adds kt*128 B).  A half-image is
// staged by 512 threads x 16 B x 2 rounds; round r, thread tid covers image
// byte off = r*8192 + tid*16.
//
// PERM (the W operand of the non-dropout kernels): image row j takes source
// row (j & ~63) + 4*(j & 15) + ((j >> 4) & 3) instead of row j.
// The image, its swizzle and every read of it are the same; a fragment row
// 16*ni + lo now holds column 4*lo + ni. A lane still reads 16 contiguous
// bytes and 8 lanes one 128-byte row segment.
template <bool MGUARD, bool PERM = false>
__device__ __forceinline__ const bf16* stage_base(const bf16* __restrict__ gsrc,
                                                  int64_t ldg, int row0, int rows_total,
                                                  int round, int tid) {
  const int off = round * 8192 + tid * 16;
  const int row = off >> 7;
  const int chunk = ((off >> 4) & 7) ^ (row & 7);
  int grow = row0 + (PERM ? (row & ~63) + 4 * (row & 15) + ((row >> 4) & 3) : row);
  if (MGUARD) grow = grow < rows_total ? grow : rows_total - 1;
  return gsrc + (int64_t)grow * ldg + chunk * 8;
}

__device__ __forceinline__ bf16x8_t lds_frag8p(const char* base, int byte_off) {
  return *reinterpret_cast<const bf16x8_t*>(base + byte_off);
}

__device__ __forceinline__ int frag_off(int row, int chunk) {
  return (row << 7) + ((chunk ^ (row & 7)) << 4);
}

template <int ACT, bool HAS_BIAS, bool HAS_RES, int SAVE, bool MGUARD, int GRADM = GRADM_NONE,
          bool FP8O = false, bool DROP = false>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_nt_8p_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ W, const void* __restrict__ bias,
    int bias_bf16, const bf16* __restrict__ res, bf16* __restrict__ Y, bf16* __restrict__ Z,
    int M, int N, int K, unsigned char* __restrict__ Y8 = nullptr,
    const float* __restrict__ scale8 = nullptr,
    unsigned int* __restrict__ amax_bits = nullptr, drop_args drop = {}) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // A images: [buf 0..1][half 0..1] at (buf*2+half)*16 KiB;
  // B images: [slot 0..2][half 0..1] at 64 KiB + (slot*2+half)*16 KiB.
  auto As = [&](int buf, int h) { return smem + (buf * 2 + h) * HALF_BYTES; };
  auto Bs = [&](int slot, int h) {
    return smem + 4 * HALF_BYTES + (slot * 2 + h) * HALF_BYTES;
  };

  // column mapping of a lane's accumulators (file header)
  constexpr bool PERM = !DROP;

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

  const int nk = K / BK;
  // Per-lane staging source bases: [half][round] per operand.
  const bf16* asrc[2][2];
  const bf16* bsrc[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      asrc[h][r] = stage_base<MGUARD>(X, K, m0 + h * 128, M, r, tid);
      bsrc[h][r] = stage_base<false, PERM>(W + (int64_t)n0 * K, K, h * 128, N, r, tid);
    }
  const int ldst = tid * 16;  // lds dest byte of round 0
  auto stageA = [&](int kt, int h) {
    char* img = As(kt & 1, h);
    glds16(asrc[h][0] + (int64_t)kt * BK, img + ldst);
    glds16(asrc[h][1] + (int64_t)kt * BK, img + 8192 + ldst);
  };
  auto stageB = [&](int kt, int slot, int h) {
    char* img = Bs(slot, h);
    glds16(bsrc[h][0] + (int64_t)kt * BK, img + ldst);
    glds16(bsrc[h][1] + (int64_t)kt * BK, img + 8192 + ldst);
  };

  // Per-lane fragment read byte offsets (loop-invariant).  A-frag (mi, kh):
  // row wm*64+16mi+lo, chunk 4kh+hi.  B-frag (ni, kh): the wave's 64 cols
  // live in B-half (wn>>1) at local rows (wn&1)*64 + 16ni + lo.
  int offA[2][4], offB[2][4];
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
      offA[kh][mi] = frag_off(wm * 64 + 16 * mi + lo, 4 * kh + hi);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      offB[kh][ni] = frag_off((wn & 1) * 64 + 16 * ni + lo, 4 * kh + hi);
  }
  const int bh = wn >> 1;  // this wave's B half

  // Prologue: stage tile 0 (B0,B1,A0,A1), certify all but A1.
  stageB(0, 0, 0);
  stageB(0, 0, 1);
  stageA(0, 0);
  stageA(0, 1);
  asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  raw_barrier();

  int slot = 0, slot1 = nk > 1 ? 1 : 0;  // B slots of tiles t, t+1
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    const char* a0i = As(buf, 0);
    const char* a1i = As(buf, 1);
    const char* bi = Bs(slot, bh);
    const bool more = t + 1 < nk;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      // ---- pr = 0 phase: read A0-frags + B-frags(kh), stage, MFMA ----
      bf16x8_t xa[4], wb[4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) xa[mi] = lds_frag8p(a0i, offA[kh][mi]);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) wb[ni] = lds_frag8p(bi, offB[kh][ni]);
      if (more) {
        if (kh == 0) stageB(t + 1, slot1, 0);
        else stageA(t + 1, 0);
      }
      if (kh == 0) {
        if (t == nk - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      }
      raw_barrier();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[0][mi][ni] = MFMA16(xa[mi], wb[ni], acc[0][mi][ni]);
      __builtin_amdgcn_s_setprio(0);

      // ---- pr = 1 phase: read A1-frags, REUSE B-frags, stage, MFMA ----
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) xa[mi] = lds_frag8p(a1i, offA[kh][mi]);
      if (more) {
        if (kh == 0) stageB(t + 1, slot1, 1);
        else stageA(t + 1, 1);
      }
      if (kh == 0) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      raw_barrier();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[1][mi][ni] = MFMA16(xa[mi], wb[ni], acc[1][mi][ni]);
      __builtin_amdgcn_s_setprio(0);
    }
    slot = slot1;
    slot1 = slot1 + 1 == 3 ? 0 : slot1 + 1;
  }

  // Epilogue: acc[pr][mi][ni] -> rows m0 + pr*128 + wm*64 + 16mi + hi*4 + r,
  // cols n0 + wn*64 + 4lo + ni (PERM) or n0 + wn*64 + 16ni + lo (DROP).
  float rs8 = 1.f, tmax = 0.f;
  if (FP8O) rs8 = fast_rcpf(scale8[0]);
  // a lane owns 4 columns (n depends on ni alone): its bias values, once
  float bv[4] = {};
  if (HAS_BIAS) {
    if constexpr (PERM) {
      load_bias4(bias, n0 + wn * 64 + 4 * lo, bias_bf16, bv);
    } else {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        bv[ni] = load_bias(bias, n0 + wn * 64 + 16 * ni + lo, bias_bf16);
    }
  }
  if constexpr (DROP) {
    // A lane's 16 elements of a fragment are rows hi*4 + {0..3} x columns
    // 16*ni + lo of the wave's 64-column group: the 4 words x 2 halves of two
    // Philox calls (one per row pair), every word used, nothing crosses lanes.
    const drop_key dkey = load_drop_key(drop);
    const unsigned cgroup = ((n0 >> 6) + wn) * 16 + lo;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
        for (int rp = 0; rp < 2; ++rp) {
          const int mb = m0 + pr * 128 + wm * 64 + 16 * mi + hi * 4 + 2 * rp;
          if (MGUARD && mb >= M) continue;
          float dm[2][4];
          drop_mults(drop, dkey, (unsigned)mb >> 1, cgroup, dm);
#pragma unroll
          for (int rr = 0; rr < 2; ++rr) {
            const int m = mb + rr;
            if (MGUARD && m >= M) continue;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
              const int n = n0 + wn * 64 + 16 * ni + lo;
              gemm_epilogue<ACT, HAS_BIAS, HAS_RES, SAVE, GRADM, FP8O, true>(
                  acc[pr][mi][ni][2 * rp + rr], m, n, N, bv[ni], res, Y, Z, Y8, rs8, &tmax,
                  dm[rr][ni]);
            }
          }
        }
      }
    }
  } else {
    // a row's 4 values of a lane are 4 consecutive columns: one call, one
    // 8-byte access per stream
    const int n = n0 + wn * 64 + 4 * lo;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + pr * 128 + wm * 64 + 16 * mi + hi * 4 + r;
          if (MGUARD && m >= M) continue;
          const float v4[4] = {acc[pr][mi][0][r], acc[pr][mi][1][r], acc[pr][mi][2][r],
                               acc[pr][mi][3][r]};
          gemm_epilogue4<ACT, HAS_BIAS, HAS_RES, SAVE, GRADM, FP8O>(v4, m, n, N, bv, res, Y, Z,
                                                                    Y8, rs8, &tmax);
        }
      }
    }
  }
  if (FP8O) {
    tmax = wave_reduce_max(tmax);
    if (lane == 0) atomicMax(amax_bits, __float_as_uint(tmax));
  }
}

}  // namespace

bool gemm8p_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && (N % BN == 0) && (K % BK == 0) && K >= 2 * BK;
}

namespace {

// One launch of a gemm_nt_8p_kernel instantiation: 160 KiB of LDS (the full
// CU), one workgroup per 256x256 output tile.
template <auto Kernel, bool WIDE = true>
void launch_8p(const torch::Tensor& x, const torch::Tensor& w, const void* biasp, int bias_bf16,
               const bf16* resp, torch::Tensor& y, bf16* zp, unsigned char* y8p = nullptr,
               const float* scale8p = nullptr, unsigned int* amaxp = nullptr,
               drop_args drop = {}) {
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  // the 4-wide epilogue's vector accesses (N % 256 == 0 keeps every row and
  // column offset a multiple of the access; the bases are the callers'). WIDE
  // is false for the dropout kernels, whose accesses stay 2 bytes wide.
  if (WIDE) {
    auto aligned = [](const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; };
    TORCH_CHECK(aligned(y.data_ptr(), 8) && aligned(resp, 8) && aligned(zp, 8) && aligned(y8p, 4),
                "8-phase GEMM: y, residual / z / g and the saved tensor must be 8-byte aligned, "
                "the e4m3 output 4-byte aligned");
    TORCH_CHECK(aligned(biasp, bias_bf16 ? 8 : 16),
                "8-phase GEMM: a bf16 bias must be 8-byte, an fp32 bias 16-byte aligned");
  }
  constexpr size_t shmem = 10 * HALF_BYTES;
  const int mt = (M + BM - 1) / BM;
  launch_lds<Kernel>(dim3(mt * (N / BN)), dim3(NTHREADS), shmem, shmem,
                     at::hip::getCurrentHIPStream(), reinterpret_cast<const bf16*>(x.data_ptr()),
                     reinterpret_cast<const bf16*>(w.data_ptr()), biasp, bias_bf16, resp,
                     reinterpret_cast<bf16*>(y.data_ptr()), zp, M, N, K, y8p, scale8p, amaxp,
                     drop);
}

// dz = (dy @ wt^T as NT on pre-transposed wt [in_f, out_f]) * act'(z) —
// the dX GEMM of an activated linear with the activation backward fused
// into the epilogue (saves the separate act_bwd elementwise pass).  With
// scale8/amax also the fused delayed-scaled e4m3 emission of dz (producer of
// the downstream fp8 dX GEMM); returns {dz bf16} or {dz bf16, dz8 e4m3 bytes}.
std::vector<torch::Tensor> gradact_8p(torch::Tensor dy, torch::Tensor wt, torch::Tensor z,
                                      const std::string& act,
                                      c10::optional<torch::Tensor> scale8,
                                      c10::optional<torch::Tensor> amax) {
  const int M = dy.size(0), K = dy.size(1), N = wt.size(0);
  TORCH_CHECK(dy.is_contiguous() && wt.is_contiguous() && z.is_contiguous());
  TORCH_CHECK(wt.size(1) == K && z.size(0) == M && z.size(1) == N);
  TORCH_CHECK(gemm8p_supported(M, N, K));
  TORCH_CHECK(!act.empty(), "gradact needs an activation, got ", act);
  const bool fp8 = scale8.has_value();
  auto y = torch::empty({M, N}, dy.options());
  torch::Tensor y8;
  if (fp8) y8 = torch::empty({M, N}, dy.options().dtype(torch::kUInt8));
  unsigned char* y8p = fp8 ? y8.data_ptr<unsigned char>() : nullptr;
  const float* scale8p = fp8 ? scale8->data_ptr<float>() : nullptr;
  unsigned int* amaxp = fp8 ? reinterpret_cast<unsigned int*>(amax->data_ptr()) : nullptr;
  const bf16* zp = reinterpret_cast<const bf16*>(z.data_ptr());
  with_act(act_code(act), [&](auto act_c) {
    with_flags(
        [&](auto mg, auto fp8_c) {
          constexpr int A = decltype(act_c)::value;
          if constexpr (A != ACT_NONE)
            launch_8p<gemm_nt_8p_kernel<A, false, true, SAVE_NONE, decltype(mg)::value, GRADM_ACT,
                                        decltype(fp8_c)::value>>(dy, wt, nullptr, 0, zp, y,
                                                                 nullptr, y8p, scale8p, amaxp);
        },
        (M % BM) != 0, fp8);
  });
  if (fp8) return {y, y8};
  return {y};
}

}  // namespace

torch::Tensor gemm_nt_8p_gradact(torch::Tensor dy, torch::Tensor wt, torch::Tensor z,
                                 std::string act) {
  return gradact_8p(dy, wt, z, act, c10::nullopt, c10::nullopt)[0];
}

std::vector<torch::Tensor> gemm_nt_8p_gradact_fp8(torch::Tensor dy, torch::Tensor wt,
                                                  torch::Tensor z, std::string act,
                                                  torch::Tensor scale8, torch::Tensor amax) {
  return gradact_8p(dy, wt, z, act, scale8, amax);
}

// dz = (dy @ wt^T) * g with g the fp16 activation derivative a SAVE_GRAD
// forward stored: the gradact GEMM with the multiplier read instead of
// computed (no activation code in the epilogue).
torch::Tensor gemm_nt_8p_gradmul(torch::Tensor dy, torch::Tensor wt, torch::Tensor g) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && wt.is_contiguous() && g.is_contiguous());
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 && wt.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(g.scalar_type() == torch::kFloat16, "gradmul needs an fp16 multiplier");
  TORCH_CHECK(dy.dim() == 2 && wt.dim() == 2 && g.dim() == 2);
  const int M = dy.size(0), K = dy.size(1), N = wt.size(0);
  TORCH_CHECK(wt.size(1) == K && g.size(0) == M && g.size(1) == N);
  TORCH_CHECK(gemm8p_supported(M, N, K));
  auto y = torch::empty({M, N}, dy.options());
  const bf16* gp = reinterpret_cast<const bf16*>(g.data_ptr());
  with_flags(
      [&](auto mg) {
        launch_8p<gemm_nt_8p_kernel<ACT_NONE, false, true, SAVE_NONE, decltype(mg)::value,
                                    GRADM_MUL>>(dy, wt, nullptr, 0, gp, y, nullptr);
      },
      (M % BM) != 0);
  return y;
}

// bias: fp32 or bf16, read as it is. save: SAVE_*; z receives what it names.
// drop (nullptr = none): dropout fused into the epilogue, for the two forms
// the MLP has: fc1 (activation, bias, no residual, SAVE_GRAD) and fc2 (no
// activation, bias, residual, SAVE_NONE).
void gemm_nt_8p(torch::Tensor x, torch::Tensor w, c10::optional<torch::Tensor> bias,
                std::string act, c10::optional<torch::Tensor> residual, torch::Tensor y,
                int save, c10::optional<torch::Tensor> z, const drop_args* drop) {
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(gemm8p_supported(M, N, K));
  TORCH_CHECK((save != SAVE_NONE) == z.has_value());
  // s * act' must stay an fp16: act' <= 1.13
  TORCH_CHECK(!drop || save != SAVE_GRAD || drop->scale * 1.25f < 65504.f,
              "dropout epilogue: the scaled derivative overflows fp16 at this p");
  const bf16* resp = residual ? reinterpret_cast<const bf16*>(residual->data_ptr()) : nullptr;
  const void* biasp = bias ? bias->data_ptr() : nullptr;
  const int bias_bf16 = bias && bias->scalar_type() == torch::kBFloat16;
  TORCH_CHECK(!bias || bias_bf16 || bias->scalar_type() == torch::kFloat32);
  bf16* zp = z ? reinterpret_cast<bf16*>(z->data_ptr()) : nullptr;
  with_act(act_code(act), [&](auto act_c) {
    with_save(save, [&](auto save_c) {
      with_flags(
          [&](auto hb, auto hr, auto mg) {
            constexpr int A = decltype(act_c)::value, S = decltype(save_c)::value;
            constexpr bool HB = decltype(hb)::value, HR = decltype(hr)::value;
            constexpr bool fc1 = A != ACT_NONE && HB && !HR && S == SAVE_GRAD;
            constexpr bool fc2 = A == ACT_NONE && HB && HR && S == SAVE_NONE;
            if constexpr (S == SAVE_GRAD && A == ACT_NONE) {
              TORCH_CHECK(false, "saving the activation derivative needs an activation");
            } else if (drop) {
              if constexpr (fc1 || fc2) {
                launch_8p<gemm_nt_8p_kernel<A, true, HR, S, decltype(mg)::value, GRADM_NONE,
                                            false, true>,
                          false>(x, w, biasp, bias_bf16, resp, y, zp, nullptr, nullptr, nullptr,
                                 *drop);
              } else {
                TORCH_CHECK(false, "dropout epilogue: only act + bias + saved derivative (fc1) "
                                   "or bias + residual (fc2)");
              }
            } else {
              launch_8p<gemm_nt_8p_kernel<A, decltype(hb)::value, decltype(hr)::value, S,
                                          decltype(mg)::value>>(x, w, biasp, bias_bf16, resp, y,
                                                                zp);
            }
          },
          bias.has_value(), residual.has_value(), (M % BM) != 0);
    });
  });
}
