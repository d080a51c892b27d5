// K12 — fused similarity-head loss kernels: the (B_local, B_global) logit
// block of the CLIP / SigLIP losses is computed tile by tile on the MFMA
// units and consumed in the epilogue; it is never stored.
//
// Main loop: acc = A @ B^T for A (M, D), B (N, D), contiguous bf16, D % 64 == 0,
// any M, N >= 1. The geometry is gemm.hip's: 128x128 tiles, BK = 64, 4 waves
// of 64x64, v_mfma_f32_16x16x32_bf16; the global_load_lds / XOR-swizzled form
// when M % 128 == 0 and N % 128 == 0, the guarded register-staged form (rows
// beyond M or N staged as zeros) otherwise. This file keeps its own copy of
// the two K loops; gemm.hip is untouched.
//
// Accumulator layout (gemm.hip, epilogue): lane (lo = lane & 15, hi = lane >> 4)
// holds acc[mi][ni][r] = row wm + 16*mi + 4*hi + r, column wn + 16*ni + lo.
// One row's 64 columns inside a wave are 4 values in each of the 16 lanes of
// one hi group: a row reduction is 4 local values and an xor-shuffle over
// 1, 2, 4, 8. Nothing crosses waves, nothing goes through LDS: the reduction
// unit is one row x one 64-column group.
//
// With x = scale * acc (+ bias), the label of row m at column diag0 + m:
//   sim_lse_fwd      per (row, 64-column group) max and sum exp(x - max) over
//                    the columns n < N -> workspace [M][ceil(N/64)]; pos[m] = x
//                    at the label; a second kernel (one wave per row, fixed
//                    order) merges the groups into lse[m]
//   sim_sigmoid_fwd  sum softplus(-z x), z = +1 at the label else -1: one
//                    partial per wave and tile, summed in a fixed order
//   sim_grad         recomputes the tile; r = exp(x - lse[m]) - [label]
//                    (softmax) or -z sigmoid(-z x) (sigmoid);
//                    G = bf16(coef * scale * r); per-wave partials of sum r*acc
//                    (d/dscale) and sum r (d/dbias) from the fp32 r, summed in
//                    a fixed order and multiplied by coef
// scale, bias and coef are pointers to fp32 device scalars, so a captured step
// never bakes a value in and nothing syncs. No atomics: every result is
// deterministic.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "mfma.h"

namespace {

typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int PITCH = BK + 8;  // guarded form only
constexpr size_t SHMEM_FAST = 4 * 8192 * sizeof(short);
constexpr size_t SHMEM_GUARDED = 2 * (BM + BN) * PITCH * sizeof(short);

#define SIM_SOFTMAX 0
#define SIM_SIGMOID 1

// ---------------------------------------------------------------------------
// main loop
// ---------------------------------------------------------------------------

// LDS image of the fast form: [128 rows][64 shorts], chunk c (16 B) of row r
// at byte r*128 + (c ^ (r&7))*16; the inverse swizzle goes on the source.
__device__ __forceinline__ void stage_tile_glds(const bf16* __restrict__ gsrc, int64_t ldg,
                                                short* lds_base, int tid) {
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
#pragma unroll
  for (int round = 0; round < 4; ++round) {
    const int off = round * 4096 + wave * 1024 + lane * 16;
    const int row = off >> 7;
    const int chunk = (off >> 4) & 7;
    const int src_chunk = chunk ^ (row & 7);
    glds16(gsrc + (int64_t)row * ldg + src_chunk * 8,
           reinterpret_cast<char*>(lds_base) + round * 4096 + wave * 1024);
  }
}

__device__ __forceinline__ bf16x8_t lds_read_frag(const short* base, int row, int chunk) {
  const int byte = (row << 7) + ((chunk ^ (row & 7)) << 4);
  return *reinterpret_cast<const bf16x8_t*>(reinterpret_cast<const char*>(base) + byte);
}

// Where a workgroup's tile lies and which of the (mt * nt) tiles it is.
struct tile_at {
  int m0, n0, id;
};

__device__ __forceinline__ tile_at this_tile(int M, int N) {
  const int mt = (M + BM - 1) / BM, nt = (N + BN - 1) / BN;
  const int wg = xcd_remap(blockIdx.x, mt * nt);
  return {(wg / nt) * BM, (wg % nt) * BN, wg};
}

// acc = A[m0 .. m0+128) @ B[n0 .. n0+128)^T. FAST: full tiles only.
template <bool FAST>
__device__ __forceinline__ void sim_tile(const bf16* __restrict__ A, const bf16* __restrict__ B,
                                         int M, int N, int K, int m0, int n0, char* smem,
                                         f32x4_t (&acc)[4][4]) {
  short* smem_s = reinterpret_cast<short*>(smem);
  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wave = tid / WAVE;
  const int lo = lane & 15, hi = lane >> 4;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int nk = K / BK;

  if constexpr (FAST) {
    auto as = [&](int buf) { return smem_s + buf * 8192; };
    auto bs = [&](int buf) { return smem_s + 16384 + buf * 8192; };
    stage_tile_glds(A + (int64_t)m0 * K, K, as(0), tid);
    stage_tile_glds(B + (int64_t)n0 * K, K, bs(0), tid);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int buf = kt & 1;
      if (kt + 1 < nk) {
        stage_tile_glds(A + (int64_t)m0 * K + (kt + 1) * BK, K, as(buf ^ 1), tid);
        stage_tile_glds(B + (int64_t)n0 * K + (kt + 1) * BK, K, bs(buf ^ 1), tid);
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_t xa[4], wb[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) xa[mi] = lds_read_frag(as(buf), wm + 16 * mi + lo, 4 * ks + hi);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) wb[ni] = lds_read_frag(bs(buf), wn + 16 * ni + lo, 4 * ks + hi);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = MFMA16(xa[mi], wb[ni], acc[mi][ni]);
      }
      __syncthreads();  // also drains the in-flight global_load_lds (vmcnt 0)
    }
  } else {
    short* as = smem_s;                    // [2][BM][PITCH]
    short* bs = as + 2 * BM * PITCH;       // [2][BN][PITCH]
    auto stage = [&](int buf, int k0) {
      short* ad = as + buf * BM * PITCH;
      short* bd = bs + buf * BN * PITCH;
      const int row = tid / 2;
      const int c0 = (tid & 1) * 32;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int cc = c0 + h * 16;
        if (m0 + row < M) {
          *reinterpret_cast<bf16x8_t*>(ad + row * PITCH + cc) =
              *reinterpret_cast<const bf16x8_t*>(A + (int64_t)(m0 + row) * K + k0 + cc);
          *reinterpret_cast<bf16x8_t*>(ad + row * PITCH + cc + 8) =
              *reinterpret_cast<const bf16x8_t*>(A + (int64_t)(m0 + row) * K + k0 + cc + 8);
        } else {
          for (int i = 0; i < 16; ++i) ad[row * PITCH + cc + i] = 0;
        }
        if (n0 + row < N) {
          *reinterpret_cast<bf16x8_t*>(bd + row * PITCH + cc) =
              *reinterpret_cast<const bf16x8_t*>(B + (int64_t)(n0 + row) * K + k0 + cc);
          *reinterpret_cast<bf16x8_t*>(bd + row * PITCH + cc + 8) =
              *reinterpret_cast<const bf16x8_t*>(B + (int64_t)(n0 + row) * K + k0 + cc + 8);
        } else {
          for (int i = 0; i < 16; ++i) bd[row * PITCH + cc + i] = 0;
        }
      }
    };
    stage(0, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int buf = kt & 1;
      if (kt + 1 < nk) stage(buf ^ 1, (kt + 1) * BK);
      const short* ad = as + buf * BM * PITCH;
      const short* bd = bs + buf * BN * PITCH;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_t xa[4], wb[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
          xa[mi] = *reinterpret_cast<const bf16x8_t*>(ad + (wm + 16 * mi + lo) * PITCH + 32 * ks + hi * 8);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          wb[ni] = *reinterpret_cast<const bf16x8_t*>(bd + (wn + 16 * ni + lo) * PITCH + 32 * ks + hi * 8);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = MFMA16(xa[mi], wb[ni], acc[mi][ni]);
      }
      __syncthreads();
    }
  }
}

// Reductions over the 16 lanes that share hi (one row's 64 columns).
__device__ __forceinline__ float row_reduce_max(float v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
  return v;
}

__device__ __forceinline__ float row_reduce_sum(float v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// ---------------------------------------------------------------------------
// softmax forward: per (row, 64-column group) max / sum-exp, pos
// ---------------------------------------------------------------------------

template <bool FAST>
__global__ __launch_bounds__(256) void sim_lse_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B, const float* __restrict__ scale_p,
    float2* __restrict__ part, float* __restrict__ pos, int M, int N, int K, int ng,
    int64_t diag0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const tile_at t = this_tile(M, N);
  f32x4_t acc[4][4] = {};
  sim_tile<FAST>(A, B, M, N, K, t.m0, t.n0, smem, acc);

  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const int lo = lane & 15, hi = lane >> 4;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const float s = *scale_p;
  // this wave's column group; the second group of the last tile lies wholly
  // beyond N when ceil(N/64) is odd (g == ng): reduced like any other (no
  // column is valid: max -inf, sum 0, no inf - inf is formed) and not stored
  const int g = (t.n0 + wn) >> 6;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = t.m0 + wm + 16 * mi + hi * 4 + r;
      float x[4];
      float mx = -INFINITY;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        x[ni] = s * acc[mi][ni][r];
        if (t.n0 + wn + 16 * ni + lo < N) mx = fmaxf(mx, x[ni]);
      }
      mx = row_reduce_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int n = t.n0 + wn + 16 * ni + lo;
        // a valid column makes mx finite; an invalid one adds nothing
        if (n < N) sum += __expf(x[ni] - mx);
        if (m < M && n < N && n == diag0 + m) pos[m] = x[ni];
      }
      sum = row_reduce_sum(sum);
      if (lo == 0 && m < M && g < ng) part[(int64_t)m * ng + g] = make_float2(mx, sum);
    }
  }
}

// lse[m] from the ng (max, sum) pairs of row m: one wave per row; lane l
// folds groups l, l + 64, ... in order, then a 6-level butterfly (both sides
// of a pair compute the same commutative merge, so all lanes agree).
__global__ void sim_lse_merge_kernel(const float2* __restrict__ part, float* __restrict__ lse,
                                     int M, int ng) {
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int wpb = blockDim.x / WAVE;
  for (int64_t m = (int64_t)blockIdx.x * wpb + wave; m < M; m += (int64_t)gridDim.x * wpb) {
    float mx = -INFINITY, sum = 0.f;
    for (int g = lane; g < ng; g += WAVE) {
      const float2 p = part[m * ng + g];
      const float nm = fmaxf(mx, p.x);  // p.x is finite: every stored group has a column
      sum = sum * __expf(mx - nm) + p.y * __expf(p.x - nm);
      mx = nm;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float om = __shfl_xor(mx, off, WAVE), os = __shfl_xor(sum, off, WAVE);
      const float nm = fmaxf(mx, om);
      if (nm > -INFINITY) sum = sum * __expf(mx - nm) + os * __expf(om - nm);
      mx = nm;
    }
    if (lane == 0) lse[m] = mx + __logf(sum);
  }
}

// ---------------------------------------------------------------------------
// sigmoid forward: sum softplus(-z x)
// ---------------------------------------------------------------------------

template <bool FAST>
__global__ __launch_bounds__(256) void sim_sigmoid_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B, const float* __restrict__ scale_p,
    const float* __restrict__ bias_p, float* __restrict__ parts, int M, int N, int K,
    int64_t diag0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const tile_at t = this_tile(M, N);
  f32x4_t acc[4][4] = {};
  sim_tile<FAST>(A, B, M, N, K, t.m0, t.n0, smem, acc);

  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const int lo = lane & 15, hi = lane >> 4;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const float s = *scale_p, b = *bias_p;
  float total = 0.f;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = t.m0 + wm + 16 * mi + hi * 4 + r;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int n = t.n0 + wn + 16 * ni + lo;
        if (m >= M || n >= N) continue;
        const float x = s * acc[mi][ni][r] + b;
        // -logsigmoid(z x) = log(1 + exp(-z x)), stable form (losses.hip)
        const float tt = (n == diag0 + m) ? -x : x;
        total += (tt > 0.f ? tt : 0.f) + __logf(1.f + __expf(-fabsf(tt)));
      }
    }
  }
  total = wave_reduce_sum(total);
  if (lane == 0) parts[t.id * 4 + wave] = total;
}

// ---------------------------------------------------------------------------
// backward: G = bf16(coef * scale * r) and the scale / bias gradient partials
// ---------------------------------------------------------------------------

template <bool FAST, int MODE>
__global__ __launch_bounds__(256) void sim_grad_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B, const float* __restrict__ scale_p,
    const float* __restrict__ bias_p, const float* __restrict__ lse,
    const float* __restrict__ coef_p, bf16* __restrict__ G, float* __restrict__ parts_s,
    float* __restrict__ parts_b, int M, int N, int K, int64_t diag0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const tile_at t = this_tile(M, N);
  f32x4_t acc[4][4] = {};
  sim_tile<FAST>(A, B, M, N, K, t.m0, t.n0, smem, acc);

  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const int lo = lane & 15, hi = lane >> 4;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const float s = *scale_p;
  const float b = bias_p ? *bias_p : 0.f;
  const float gs = *coef_p * s;
  float ds = 0.f, db = 0.f;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = t.m0 + wm + 16 * mi + hi * 4 + r;
      if (m >= M) continue;
      float l = 0.f;
      if (MODE == SIM_SOFTMAX) l = lse[m];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int n = t.n0 + wn + 16 * ni + lo;
        if (n >= N) continue;
        const float a = acc[mi][ni][r];
        const float x = s * a + b;
        const bool label = n == diag0 + m;
        float rr;
        if (MODE == SIM_SOFTMAX) {
          rr = __expf(x - l) - (label ? 1.f : 0.f);
        } else {
          // -z sigmoid(-z x) = -z / (1 + exp(z x)); exp overflow gives -z / inf = 0
          const float z = label ? 1.f : -1.f;
          rr = -z * fast_rcpf(1.f + __expf(z * x));
        }
        G[(int64_t)m * N + n] = f2bf(gs * rr);
        ds += rr * a;
        db += rr;
      }
    }
  }
  ds = wave_reduce_sum(ds);
  db = wave_reduce_sum(db);
  if (lane == 0) {
    parts_s[t.id * 4 + wave] = ds;
    parts_b[t.id * 4 + wave] = db;
  }
}

// out[k] = (coef ? *coef : 1) * sum(parts[k*n .. k*n + n)), one block per k,
// in a fixed order: thread-strided sums, the wave butterfly, then the 4 waves.
__global__ __launch_bounds__(256) void sim_sum_parts_kernel(const float* __restrict__ parts,
                                                            int n, const float* __restrict__ coef_p,
                                                            float* __restrict__ out) {
  __shared__ float s_acc[4];
  const float* p = parts + (int64_t)blockIdx.x * n;
  float v = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) v += p[i];
  v = wave_reduce_sum(v);
  if (threadIdx.x % WAVE == 0) s_acc[threadIdx.x / WAVE] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float total = (s_acc[0] + s_acc[1]) + (s_acc[2] + s_acc[3]);
    out[blockIdx.x] = coef_p ? *coef_p * total : total;
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

struct sim_shape {
  int M, N, K, tiles;
  bool fast;
};

sim_shape check_operands(const char* op, const torch::Tensor& a, const torch::Tensor& b) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.device() == b.device(), op,
              ": a and b must be on one GPU");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 && b.scalar_type() == torch::kBFloat16, op,
              ": a and b must be bf16");
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.is_contiguous() && b.is_contiguous(), op,
              ": a (M, D) and b (N, D) must be contiguous");
  const int64_t M = a.size(0), N = b.size(0), K = a.size(1);
  TORCH_CHECK(b.size(1) == K && K % BK == 0 && K > 0, op, ": D must match and be a multiple of ",
              BK, ", got ", K, " and ", b.size(1));
  TORCH_CHECK(M >= 1 && N >= 1, op, ": empty operand");
  const int64_t tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  TORCH_CHECK(M < (1 << 30) && N < (1 << 30) && tiles < (1 << 28), op, ": shape too large");
  // 16-byte loads of both operands
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(b.data_ptr()) % 16 == 0,
              op, ": operands must be 16-byte aligned");
  return {(int)M, (int)N, (int)K, (int)tiles, M % BM == 0 && N % BN == 0};
}

const float* scalar_ptr(const char* op, const char* name, const torch::Tensor& t,
                        const torch::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() &&
                  t.scalar_type() == torch::kFloat32 && t.numel() == 1,
              op, ": ", name, " must be one fp32 element on the operands' device");
  return t.data_ptr<float>();
}

}  // namespace

bool sim_supported(int64_t M, int64_t N, int64_t D, std::string dtype) {
  return dtype == "torch.bfloat16" && M >= 1 && N >= 1 && D > 0 && D % BK == 0;
}

// (lse[M], pos[M]) of x = scale * a @ b^T; the label of row m is column
// diag0 + m, which must exist for every row.
std::vector<torch::Tensor> sim_lse_fwd(torch::Tensor a, torch::Tensor b, torch::Tensor scale,
                                       int64_t diag0) {
  const sim_shape sh = check_operands("sim_lse_fwd", a, b);
  const float* sp = scalar_ptr("sim_lse_fwd", "scale", scale, a);
  TORCH_CHECK(diag0 >= 0 && diag0 + sh.M <= sh.N, "sim_lse_fwd: labels diag0 + m = ", diag0,
              " .. ", diag0 + sh.M - 1, " must lie inside the ", sh.N, " columns");
  const int ng = (sh.N + 63) / 64;
  auto f32 = a.options().dtype(torch::kFloat32);
  auto part = torch::empty({sh.M, ng, 2}, f32);
  auto lse = torch::empty({sh.M}, f32);
  auto pos = torch::empty({sh.M}, f32);
  auto stream = at::hip::getCurrentHIPStream();
  const bf16* ap = bf16_ptr(a);
  const bf16* bp = bf16_ptr(b);
  float2* pp = reinterpret_cast<float2*>(part.data_ptr<float>());
  if (sh.fast)
    launch_lds<sim_lse_kernel<true>>(dim3(sh.tiles), dim3(256), SHMEM_FAST, SHMEM_FAST, stream,
                                     ap, bp, sp, pp, pos.data_ptr<float>(), sh.M, sh.N, sh.K,
                                     ng, diag0);
  else
    launch_lds<sim_lse_kernel<false>>(dim3(sh.tiles), dim3(256), SHMEM_GUARDED, SHMEM_GUARDED,
                                      stream, ap, bp, sp, pp, pos.data_ptr<float>(), sh.M, sh.N,
                                      sh.K, ng, diag0);
  const int grid = (int)std::min<int64_t>((sh.M + 3) / 4, 2048);
  hipLaunchKernelGGL(sim_lse_merge_kernel, dim3(grid), dim3(256), 0, stream, pp,
                     lse.data_ptr<float>(), sh.M, ng);
  return {lse, pos};
}

// loss_sum[1] = sum_mn softplus(-z (scale * a @ b^T + bias)), z = +1 at column
// diag0 + m (which may lie outside the block) else -1.
torch::Tensor sim_sigmoid_fwd(torch::Tensor a, torch::Tensor b, torch::Tensor scale,
                              torch::Tensor bias, int64_t diag0) {
  const sim_shape sh = check_operands("sim_sigmoid_fwd", a, b);
  const float* sp = scalar_ptr("sim_sigmoid_fwd", "scale", scale, a);
  const float* bp_ = scalar_ptr("sim_sigmoid_fwd", "bias", bias, a);
  auto f32 = a.options().dtype(torch::kFloat32);
  auto parts = torch::empty({(int64_t)sh.tiles * 4}, f32);
  auto out = torch::empty({1}, f32);
  auto stream = at::hip::getCurrentHIPStream();
  if (sh.fast)
    launch_lds<sim_sigmoid_kernel<true>>(dim3(sh.tiles), dim3(256), SHMEM_FAST, SHMEM_FAST,
                                         stream, bf16_ptr(a), bf16_ptr(b), sp, bp_,
                                         parts.data_ptr<float>(), sh.M, sh.N, sh.K, diag0);
  else
    launch_lds<sim_sigmoid_kernel<false>>(dim3(sh.tiles), dim3(256), SHMEM_GUARDED,
                                          SHMEM_GUARDED, stream, bf16_ptr(a), bf16_ptr(b), sp,
                                          bp_, parts.data_ptr<float>(), sh.M, sh.N, sh.K, diag0);
  hipLaunchKernelGGL(sim_sum_parts_kernel, dim3(1), dim3(256), 0, stream,
                     parts.data_ptr<float>(), sh.tiles * 4, (const float*)nullptr,
                     out.data_ptr<float>());
  return out;
}

// (G (M, N) bf16, dscale[1], dbias[1]) for one column chunk b of the block;
// mode 0 = softmax (needs lse, takes no bias), 1 = sigmoid (needs bias).
// diag0 is relative to the chunk and may be negative or past it.
std::vector<torch::Tensor> sim_grad(torch::Tensor a, torch::Tensor b, torch::Tensor scale,
                                    c10::optional<torch::Tensor> bias,
                                    c10::optional<torch::Tensor> lse, torch::Tensor coef,
                                    int64_t diag0, int64_t mode) {
  const sim_shape sh = check_operands("sim_grad", a, b);
  const float* sp = scalar_ptr("sim_grad", "scale", scale, a);
  const float* cp = scalar_ptr("sim_grad", "coef", coef, a);
  TORCH_CHECK(mode == SIM_SOFTMAX || mode == SIM_SIGMOID, "sim_grad: bad mode ", mode);
  const float* bp_ = nullptr;
  const float* lp = nullptr;
  if (mode == SIM_SOFTMAX) {
    TORCH_CHECK(lse.has_value() && !bias.has_value(),
                "sim_grad: the softmax mode needs lse and takes no bias");
    TORCH_CHECK(lse->is_cuda() && lse->device() == a.device() && lse->is_contiguous() &&
                    lse->scalar_type() == torch::kFloat32 && lse->numel() == sh.M,
                "sim_grad: lse must be contiguous fp32 [M]");
    lp = lse->data_ptr<float>();
  } else {
    TORCH_CHECK(bias.has_value(), "sim_grad: the sigmoid mode needs a bias");
    bp_ = scalar_ptr("sim_grad", "bias", *bias, a);
  }
  auto f32 = a.options().dtype(torch::kFloat32);
  auto G = torch::empty({sh.M, sh.N}, a.options());
  auto parts = torch::empty({2, (int64_t)sh.tiles * 4}, f32);
  auto sums = torch::empty({2}, f32);
  float* ps = parts.data_ptr<float>();
  float* pb = ps + (int64_t)sh.tiles * 4;
  auto stream = at::hip::getCurrentHIPStream();
  with_int<SIM_SOFTMAX, SIM_SIGMOID>((int)mode, "mode", [&](auto mode_c) {
    constexpr int MD = decltype(mode_c)::value;
    if (sh.fast)
      launch_lds<sim_grad_kernel<true, MD>>(dim3(sh.tiles), dim3(256), SHMEM_FAST, SHMEM_FAST,
                                            stream, bf16_ptr(a), bf16_ptr(b), sp, bp_, lp, cp,
                                            bf16_ptr(G), ps, pb, sh.M, sh.N, sh.K, diag0);
    else
      launch_lds<sim_grad_kernel<false, MD>>(dim3(sh.tiles), dim3(256), SHMEM_GUARDED,
                                             SHMEM_GUARDED, stream, bf16_ptr(a), bf16_ptr(b), sp,
                                             bp_, lp, cp, bf16_ptr(G), ps, pb, sh.M, sh.N, sh.K,
                                             diag0);
  });
  hipLaunchKernelGGL(sim_sum_parts_kernel, dim3(2), dim3(256), 0, stream, ps, sh.tiles * 4, cp,
                     sums.data_ptr<float>());
  return {G, sums.slice(0, 0, 1), sums.slice(0, 1, 2)};
}
