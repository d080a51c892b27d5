// K4/K6/K7/K8 — MFMA bf16 GEMM with fused bias/activation/residual epilogue.
//
// linear_fwd computes y = act(x @ w^T + bias) [+ residual] for x (M,K)
// row-major and w (N,K) row-major (torch Linear convention) — an "NT" GEMM
// on v_mfma_f32_16x16x32_bf16 tiles.
//
// Fast path (full 128x128 tiles, K%64==0 — every hot shape in the model zoo:
// ViT/CLIP/SigLIP widths are multiples of 128 and M = B*L*? lands on
// multiples of 128 for the bench batch sizes):
//   * 128x128 macro-tile, BK=64, 4 waves, 64x64 per wave (4x4 fragments);
//   * async global->LDS staging via __builtin_amdgcn_global_load_lds
//     width 16 (CDNA guide §5 ladder step 3: +69% over register staging);
//   * LDS image XOR-swizzled (chunk ^= row&7, 16B chunks) with the inverse
//     swizzle applied to the per-lane SOURCE address (guide rule 21) so the
//     ds_read_b128 fragment reads are bank-conflict-free;
//   * double-buffered LDS; stage(t+1) issued BEFORE compute(t) (minimum
//     2-phase recipe); __syncthreads() drains the in-flight DMA (vmcnt(0)
//     is emitted by the compiler with a glds outstanding);
//   * XCD-aware bijective blockIdx remap (guide T1) for L2 tile locality.
//
// Ragged shapes fall back to the generic guarded kernel below.
//
// linear_fwd sends every shape the 8-phase 256x256-tile kernel supports
// (gemm8p.hip: N%256==0, K>=128, any M) there; the two kernels in this file
// take the rest: N%256!=0 (SigLIP-so400m's 1152), ragged N, or K==64.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "mfma.h"

namespace {

typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int PITCH = BK + 8;  // generic path only

// ---------------------------------------------------------------------------
// fast path: 128x128, glds staging, swizzled LDS
// ---------------------------------------------------------------------------

// LDS linear image: [128 rows][64 shorts] = 128 B/row, 16 KiB per operand
// tile; chunk c (16 B) of row r lives at byte r*128 + (c ^ (r&7))*16.

__device__ __forceinline__ void stage_tile_glds(const bf16* __restrict__ gsrc, int64_t ldg,
                                                short* lds_base, int tid) {
  // 256 threads stage 128x64 shorts (16 KiB): 4 rounds of 4 KiB; each wave
  // writes 1 KiB linearly at (round*4K + wave*1K); lane l covers offset
  // l*16. Source address carries the inverse swizzle.
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
#pragma unroll
  for (int round = 0; round < 4; ++round) {
    const int off = round * 4096 + wave * 1024 + lane * 16;  // byte offset in image
    const int row = off >> 7;              // /128
    const int chunk = (off >> 4) & 7;      // 16B chunk within row
    const int src_chunk = chunk ^ (row & 7);
    glds16(gsrc + (int64_t)row * ldg + src_chunk * 8,
           reinterpret_cast<char*>(lds_base) + round * 4096 + wave * 1024);
  }
}

__device__ __forceinline__ bf16x8_t lds_read_frag(const short* base, int row, int chunk) {
  const int byte = (row << 7) + ((chunk ^ (row & 7)) << 4);
  return *reinterpret_cast<const bf16x8_t*>(reinterpret_cast<const char*>(base) + byte);
}

template <int ACT, bool HAS_BIAS, bool HAS_RES, int SAVE>
__global__ __launch_bounds__(256) void gemm_nt_fast_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ W, const void* __restrict__ bias,
    int bias_bf16, const bf16* __restrict__ res, bf16* __restrict__ Y, bf16* __restrict__ Z,
    int M, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* smem_s = reinterpret_cast<short*>(smem);
  // buffers: x tiles at [0,8192) and [8192,16384); w tiles at +16384
  auto xs = [&](int buf) { return smem_s + buf * 8192; };
  auto ws = [&](int buf) { return smem_s + 16384 + buf * 8192; };

  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wave = tid / WAVE;
  const int lo = lane & 15, hi = lane >> 4;

  // XCD-aware bijective remap of the linear tile id (guide T1)
  const int mt = M / BM, nt = N / BN;
  const int wg = xcd_remap(blockIdx.x, mt * nt);
  const int m0 = (wg / nt) * BM;
  const int n0 = (wg % nt) * BN;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

  f32x4_t acc[4][4] = {};

  stage_tile_glds(X + (int64_t)m0 * K, K, xs(0), tid);
  stage_tile_glds(W + (int64_t)n0 * K, K, ws(0), tid);
  __syncthreads();

  const int nk = K / BK;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) {
      stage_tile_glds(X + (int64_t)m0 * K + (kt + 1) * BK, K, xs(buf ^ 1), tid);
      stage_tile_glds(W + (int64_t)n0 * K + (kt + 1) * BK, K, ws(buf ^ 1), tid);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t xa[4], wb[4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) xa[mi] = lds_read_frag(xs(buf), wm + 16 * mi + lo, 4 * ks + hi);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) wb[ni] = lds_read_frag(ws(buf), wn + 16 * ni + lo, 4 * ks + hi);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = MFMA16(xa[mi], wb[ni], acc[mi][ni]);
    }
    __syncthreads();  // also drains the in-flight global_load_lds (vmcnt 0)
  }

  // epilogue: C rows = m (hi*4+r of each 16-fragment), col = n (lo); a lane
  // owns 4 columns, so its 4 bias values are loaded once
  float bv[4] = {};
  if (HAS_BIAS) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) bv[ni] = load_bias(bias, n0 + wn + 16 * ni + lo, bias_bf16);
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm + 16 * mi + hi * 4 + r;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int n = n0 + wn + 16 * ni + lo;
        gemm_epilogue<ACT, HAS_BIAS, HAS_RES, SAVE>(acc[mi][ni][r], m, n, N, bv[ni], res, Y, Z);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// generic (ragged) path — guarded staging, padded LDS, register staging
// ---------------------------------------------------------------------------

template <int ACT, bool HAS_BIAS, bool HAS_RES, int SAVE>
__global__ __launch_bounds__(256) void gemm_nt_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ W, const void* __restrict__ bias,
    int bias_bf16, const bf16* __restrict__ res, bf16* __restrict__ Y, bf16* __restrict__ Z,
    int M, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* xs = reinterpret_cast<short*>(smem);              // [2][BM][PITCH]
  short* ws = xs + 2 * BM * PITCH;                         // [2][BN][PITCH]

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int lo = lane & 15, hi = lane >> 4;

  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int wm = (wave >> 1) * 64;
  const int wn = (wave & 1) * 64;

  f32x4_t acc[4][4] = {};

  auto stage = [&](int buf, int k0) {
    short* xd = xs + buf * BM * PITCH;
    short* wd = ws + buf * BN * PITCH;
    const int row = tid / 2;
    const int c0 = (tid & 1) * 32;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int cc = c0 + h * 16;
      if (m0 + row < M) {
        *reinterpret_cast<bf16x8_t*>(xd + row * PITCH + cc) =
            *reinterpret_cast<const bf16x8_t*>(X + (int64_t)(m0 + row) * K + k0 + cc);
        *reinterpret_cast<bf16x8_t*>(xd + row * PITCH + cc + 8) =
            *reinterpret_cast<const bf16x8_t*>(X + (int64_t)(m0 + row) * K + k0 + cc + 8);
      } else {
        for (int i = 0; i < 16; ++i) xd[row * PITCH + cc + i] = 0;
      }
      if (n0 + row < N) {
        *reinterpret_cast<bf16x8_t*>(wd + row * PITCH + cc) =
            *reinterpret_cast<const bf16x8_t*>(W + (int64_t)(n0 + row) * K + k0 + cc);
        *reinterpret_cast<bf16x8_t*>(wd + row * PITCH + cc + 8) =
            *reinterpret_cast<const bf16x8_t*>(W + (int64_t)(n0 + row) * K + k0 + cc + 8);
      } else {
        for (int i = 0; i < 16; ++i) wd[row * PITCH + cc + i] = 0;
      }
    }
  };

  stage(0, 0);
  __syncthreads();

  const int nk = K / BK;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) stage(buf ^ 1, (kt + 1) * BK);
    short* xd = xs + buf * BM * PITCH;
    short* wd = ws + buf * BN * PITCH;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t xa[4], wb[4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        xa[mi] = *reinterpret_cast<const bf16x8_t*>(xd + (wm + 16 * mi + lo) * PITCH + 32 * ks + hi * 8);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        wb[ni] = *reinterpret_cast<const bf16x8_t*>(wd + (wn + 16 * ni + lo) * PITCH + 32 * ks + hi * 8);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = MFMA16(xa[mi], wb[ni], acc[mi][ni]);
    }
    __syncthreads();
  }

  float bv[4] = {};
  if (HAS_BIAS) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + wn + 16 * ni + lo;
      if (n < N) bv[ni] = load_bias(bias, n, bias_bf16);
    }
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm + 16 * mi + hi * 4 + r;
      if (m >= M) continue;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int n = n0 + wn + 16 * ni + lo;
        if (n >= N) continue;
        gemm_epilogue<ACT, HAS_BIAS, HAS_RES, SAVE>(acc[mi][ni][r], m, n, N, bv[ni], res, Y, Z);
      }
    }
  }
}

}  // namespace

// 8-phase 256x256-tile kernel (gemm8p.hip)
bool gemm8p_supported(int64_t M, int64_t N, int64_t K);
void gemm_nt_8p(torch::Tensor x, torch::Tensor w, c10::optional<torch::Tensor> bias,
                std::string act, c10::optional<torch::Tensor> residual, torch::Tensor y,
                int save, c10::optional<torch::Tensor> z, const drop_args* drop);

// Shapes and dtypes linear_fwd takes (whether it is used is the caller's
// choice: JIMM_AMD_GEMM is read in Python, ops/hip_linear.py)
bool gemm_supported(int64_t M, int64_t N, int64_t K, std::string dtype) {
  return dtype == "torch.bfloat16" && K % BK == 0;
}

namespace {

// y = act(x @ w^T + bias) [+ residual] and, per `save` (SAVE_*), nothing,
// the bf16 pre-activation or the fp16 activation derivative as the second
// tensor (undefined = None in Python for SAVE_NONE).
// p > 0: dropout at `site` under the device {seed, step} pair `rng`, fused
// into the 8-phase kernel's epilogue (gemm_nt_8p names the two forms); a
// shape that kernel does not take is an error, raised before any launch.
std::vector<torch::Tensor> linear_fwd_impl(torch::Tensor x, torch::Tensor w,
                                           c10::optional<torch::Tensor> bias, std::string act,
                                           c10::optional<torch::Tensor> residual, int save,
                                           double p, c10::optional<torch::Tensor> rng,
                                           int64_t site) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && w.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && w.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2);
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && K % BK == 0);
  const unsigned thresh = drop_threshold(p);
  drop_args drop = {};
  if (thresh > 0) {
    TORCH_CHECK(gemm8p_supported(M, N, K), "linear_fwd: dropout is fused into the 8-phase "
                "kernel only, which does not take M=", M, " N=", N, " K=", K);
    drop = make_drop_args(thresh, rng, site, x);
  }
  TORCH_CHECK(save != SAVE_GRAD || !act.empty(),
              "saving the activation derivative needs an activation");
  if (residual)
    TORCH_CHECK(residual->is_contiguous() && residual->scalar_type() == torch::kBFloat16 &&
                residual->numel() == (int64_t)M * N);
  auto y = torch::empty({M, N}, x.options());
  torch::Tensor z;
  if (save == SAVE_PRE) z = torch::empty({M, N}, x.options());
  if (save == SAVE_GRAD) z = torch::empty({M, N}, x.options().dtype(torch::kFloat16));
  // The kernels read an fp32 or a bf16 bias as it is (no cast kernel per
  // call); any other dtype goes through fp32.
  c10::optional<torch::Tensor> b;
  if (bias) {
    TORCH_CHECK(bias->numel() == N);
    b = bias->contiguous();
    if (b->scalar_type() != torch::kBFloat16 && b->scalar_type() != torch::kFloat32)
      b = b->to(torch::kFloat32);
  }
  c10::optional<torch::Tensor> zopt;
  if (save != SAVE_NONE) zopt = z;

  if (gemm8p_supported(M, N, K)) {
    gemm_nt_8p(x, w, b, act, residual, y, save, zopt, thresh > 0 ? &drop : nullptr);
    return {y, z};
  }

  auto stream = at::hip::getCurrentHIPStream();
  const bf16* xp = reinterpret_cast<const bf16*>(x.data_ptr());
  const bf16* wp = reinterpret_cast<const bf16*>(w.data_ptr());
  const void* biasp = b ? b->data_ptr() : nullptr;
  const int bias_bf16 = b && b->scalar_type() == torch::kBFloat16;
  const bf16* resp = residual ? reinterpret_cast<const bf16*>(residual->data_ptr()) : nullptr;
  bf16* yp = reinterpret_cast<bf16*>(y.data_ptr());
  bf16* zp = zopt ? reinterpret_cast<bf16*>(z.data_ptr()) : nullptr;
  const bool fast = (M % BM == 0) && (N % BN == 0);
  with_act(act_code(act), [&](auto act_c) {
    with_save(save, [&](auto save_c) {
      with_flags(
          [&](auto hb, auto hr, auto fast_c) {
            constexpr int A = decltype(act_c)::value, S = decltype(save_c)::value;
            constexpr bool HB = decltype(hb)::value, HR = decltype(hr)::value;
            if constexpr (S == SAVE_GRAD && A == ACT_NONE) {
              TORCH_CHECK(false, "saving the activation derivative needs an activation");
            } else if constexpr (decltype(fast_c)::value) {
              constexpr size_t shmem = 4 * 8192 * sizeof(short);
              launch_lds<gemm_nt_fast_kernel<A, HB, HR, S>>(
                  dim3((M / BM) * (N / BN)), dim3(256), shmem, shmem, stream, xp, wp, biasp,
                  bias_bf16, resp, yp, zp, M, N, K);
            } else {
              constexpr size_t shmem = 2 * (BM + BN) * PITCH * sizeof(short);
              launch_lds<gemm_nt_kernel<A, HB, HR, S>>(
                  dim3((M + BM - 1) / BM, (N + BN - 1) / BN), dim3(256), shmem, shmem, stream,
                  xp, wp, biasp, bias_bf16, resp, yp, zp, M, N, K);
            }
          },
          bias.has_value(), residual.has_value(), fast);
    });
  });
  return {y, z};
}

}  // namespace

std::vector<torch::Tensor> linear_fwd(torch::Tensor x, torch::Tensor w,
                                      c10::optional<torch::Tensor> bias, std::string act,
                                      c10::optional<torch::Tensor> residual, bool save_z,
                                      double p, c10::optional<torch::Tensor> rng,
                                      int64_t site) {
  return linear_fwd_impl(x, w, bias, act, residual, save_z ? SAVE_PRE : SAVE_NONE, p, rng,
                         site);
}

// The forward of an activated linear that saves g = act'(x @ w^T + bias) as
// fp16 in place of the pre-activation: returns {y, g}, y bitwise what
// linear_fwd returns. gemm_nt_8p_gradmul consumes g. With p > 0 both carry the
// dropout that follows the activation: y = act(pre)*m*s, g = act'(pre)*m*s,
// so that backward needs nothing beyond the same gradmul.
std::vector<torch::Tensor> linear_fwd_actgrad(torch::Tensor x, torch::Tensor w,
                                              c10::optional<torch::Tensor> bias,
                                              std::string act,
                                              c10::optional<torch::Tensor> residual,
                                              double p, c10::optional<torch::Tensor> rng,
                                              int64_t site) {
  return linear_fwd_impl(x, w, bias, act, residual, SAVE_GRAD, p, rng, site);
}
