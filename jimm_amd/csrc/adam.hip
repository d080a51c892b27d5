// K14 — fused Adam update (optax.adam semantics:
// /root/reference/examples/vit_training.py:202-203), mixed-precision aware:
// params bf16 or fp32, moments fp32, optional fp32 master weights.
//
// Multi-tensor: the python side passes the whole parameter list; tensors are
// batched into chunk descriptors and processed by ONE kernel launch per
// ~64-tensor batch (launch-bound otherwise: ~150 params x ~1.5us).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

constexpr int kChunkSize = 1 << 16;  // elements per chunk
constexpr int kMaxChunks = 4096;

struct ChunkDesc {
  const void* g;
  void* p;
  float* m;
  float* v;
  float* master;  // nullptr if none
  int64_t offset;
  int64_t n;  // elements in this chunk
  int is_bf16;
};

__global__ void adam_kernel(const ChunkDesc* __restrict__ chunks, int nchunks, float lr,
                            float b1, float b2, float eps, float wd, float bc1, float bc2) {
  for (int ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    ChunkDesc c = chunks[ci];
    for (int64_t i = threadIdx.x; i < c.n; i += blockDim.x) {
      const int64_t idx = c.offset + i;
      float g = c.is_bf16 ? bf2f(reinterpret_cast<const bf16*>(c.g)[idx])
                          : reinterpret_cast<const float*>(c.g)[idx];
      float m = c.m[idx] = b1 * c.m[idx] + (1.f - b1) * g;
      float v = c.v[idx] = b2 * c.v[idx] + (1.f - b2) * g * g;
      float upd = (m / bc1) / (sqrtf(v / bc2) + eps);
      float w0 = c.master ? c.master[idx]
                          : (c.is_bf16 ? bf2f(reinterpret_cast<bf16*>(c.p)[idx])
                                       : reinterpret_cast<float*>(c.p)[idx]);
      if (wd != 0.f) upd += wd * w0;
      float w1 = w0 - lr * upd;
      if (c.master) c.master[idx] = w1;
      if (c.is_bf16)
        reinterpret_cast<bf16*>(c.p)[idx] = f2bf(w1);
      else
        reinterpret_cast<float*>(c.p)[idx] = w1;
    }
  }
}

// Clip stats buffer (fp32 x kStatsLen), written by clip_finalize_kernel and read
// by everything downstream, so a replayed graph takes the clip decision on the
// device: [0] pre-clip global L2 norm, [1] coef, [2] finite (1 / 0),
// [3] running count of skipped (non-finite) steps.
constexpr int kStatsLen = 4;
enum { kStatNorm = 0, kStatCoef = 1, kStatFinite = 2, kStatSkipped = 3 };

// CLIP = false is the plain update (stats unused). CLIP = true multiplies each
// loaded g by stats[coef] and leaves p/m/v/master untouched on a non-finite norm.
// omb1/omb2 are 1 - beta, rounded by the caller: adam_apply keeps the fp32
// subtraction it has always used (1.f - 0.999f is 1.3e-5 off 0.001, and its
// results must not move); the clipped path rounds the fp64 difference, as the
// eager oracle does.
template <bool CLIP>
__global__ void adam_kernel_dev(const ChunkDesc* __restrict__ chunks, int nchunks,
                                const float* __restrict__ lr_ptr,
                                const int* __restrict__ step_ptr,
                                const float* __restrict__ stats, float b1, float b2,
                                float omb1, float omb2, float eps, float wd) {
  float coef = 1.f;
  if constexpr (CLIP) {
    if (stats[kStatFinite] == 0.f) return;
    coef = stats[kStatCoef];
  }
  const float lr = *lr_ptr;
  const float st = (float)*step_ptr;
  const float bc1 = 1.f - __powf(b1, st);
  const float bc2 = 1.f - __powf(b2, st);
  constexpr int V = 4;  // vectorized: 16-B fp32 / 8-B bf16 accesses
  for (int ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    ChunkDesc c = chunks[ci];
    const int64_t nv = c.n / V;
    for (int64_t iv = threadIdx.x; iv < nv; iv += blockDim.x) {
      const int64_t idx = c.offset + iv * V;
      float g[V], m[V], v[V], w0[V], w1[V];
      if (c.is_bf16) vload_f32<V>(reinterpret_cast<const bf16*>(c.g) + idx, g);
      else vload_f32<V>(reinterpret_cast<const float*>(c.g) + idx, g);
      vload_f32<V>(c.m + idx, m);
      vload_f32<V>(c.v + idx, v);
      if (c.master) vload_f32<V>(c.master + idx, w0);
      else if (c.is_bf16) vload_f32<V>(reinterpret_cast<bf16*>(c.p) + idx, w0);
      else vload_f32<V>(reinterpret_cast<float*>(c.p) + idx, w0);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if constexpr (CLIP) g[k] *= coef;
        m[k] = b1 * m[k] + omb1 * g[k];
        v[k] = b2 * v[k] + omb2 * g[k] * g[k];
        float upd = (m[k] / bc1) / (sqrtf(v[k] / bc2) + eps);
        if (wd != 0.f) upd += wd * w0[k];
        w1[k] = w0[k] - lr * upd;
      }
      vstore_f32<V>(c.m + idx, m);
      vstore_f32<V>(c.v + idx, v);
      if (c.master) vstore_f32<V>(c.master + idx, w1);
      if (c.is_bf16) vstore_f32<V>(reinterpret_cast<bf16*>(c.p) + idx, w1);
      else vstore_f32<V>(reinterpret_cast<float*>(c.p) + idx, w1);
    }
    // scalar tail
    for (int64_t i = nv * V + threadIdx.x; i < c.n; i += blockDim.x) {
      const int64_t idx = c.offset + i;
      float g = c.is_bf16 ? bf2f(reinterpret_cast<const bf16*>(c.g)[idx])
                          : reinterpret_cast<const float*>(c.g)[idx];
      if constexpr (CLIP) g *= coef;
      float m = c.m[idx] = b1 * c.m[idx] + omb1 * g;
      float v = c.v[idx] = b2 * c.v[idx] + omb2 * g * g;
      float upd = (m / bc1) / (sqrtf(v / bc2) + eps);
      float w0 = c.master ? c.master[idx]
                          : (c.is_bf16 ? bf2f(reinterpret_cast<bf16*>(c.p)[idx])
                                       : reinterpret_cast<float*>(c.p)[idx]);
      if (wd != 0.f) upd += wd * w0;
      float w1 = w0 - lr * upd;
      if (c.master) c.master[idx] = w1;
      if (c.is_bf16)
        reinterpret_cast<bf16*>(c.p)[idx] = f2bf(w1);
      else
        reinterpret_cast<float*>(c.p)[idx] = w1;
    }
  }
}

__global__ void incr_kernel(int* __restrict__ step) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *step += 1;
}

// A skipped step must not advance bias correction.
__global__ void incr_if_finite_kernel(int* __restrict__ step, const float* __restrict__ stats) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && stats[kStatFinite] != 0.f) *step += 1;
}

// ---- global-norm gradient clipping ------------------------------------------
// Stage 1: sum of squares of every gradient chunk, ONE fp32 partial per chunk
// (indexed by chunk number, so the result does not depend on the grid size; no
// atomics). Per thread at most kChunkSize / 256 = 256 sequential fp32 adds,
// then a wave butterfly, then the 4 wave sums in wave order.
constexpr int kNormThreads = 256;

__global__ void __launch_bounds__(kNormThreads)
grad_sqnorm_kernel(const ChunkDesc* __restrict__ chunks, int nchunks,
                   float* __restrict__ partials) {
  constexpr int V = 4;
  constexpr int NW = kNormThreads / WAVE;
  __shared__ float wsum[NW];
  for (int ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    ChunkDesc c = chunks[ci];
    float acc = 0.f;
    const int64_t nv = c.n / V;
    for (int64_t iv = threadIdx.x; iv < nv; iv += blockDim.x) {
      const int64_t idx = c.offset + iv * V;
      float g[V];
      if (c.is_bf16) vload_f32<V>(reinterpret_cast<const bf16*>(c.g) + idx, g);
      else vload_f32<V>(reinterpret_cast<const float*>(c.g) + idx, g);
#pragma unroll
      for (int k = 0; k < V; ++k) acc += g[k] * g[k];
    }
    // scalar tail
    for (int64_t i = nv * V + threadIdx.x; i < c.n; i += blockDim.x) {
      const int64_t idx = c.offset + i;
      float g = c.is_bf16 ? bf2f(reinterpret_cast<const bf16*>(c.g)[idx])
                          : reinterpret_cast<const float*>(c.g)[idx];
      acc += g * g;
    }
    acc = wave_reduce_sum(acc);
    if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      float s = wsum[0];
#pragma unroll
      for (int w = 1; w < NW; ++w) s += wsum[w];
      partials[ci] = s;
    }
    __syncthreads();  // wsum is reused by the next chunk
  }
}

// Stage 2: one block adds the chunk partials of ALL param groups in fp64, in
// an order fixed by the block size alone, and publishes the clip decision.
constexpr int kFinalThreads = 256;

__global__ void __launch_bounds__(kFinalThreads)
clip_finalize_kernel(const float* __restrict__ partials, int n, float max_norm,
                     float* __restrict__ stats) {
  __shared__ double red[kFinalThreads];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += kFinalThreads) acc += (double)partials[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kFinalThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0]);
    const bool finite = isfinite(norm);
    // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1);
    // a non-finite norm keeps the raw quotient (0 for inf, NaN for NaN)
    const float q = max_norm / (norm + 1e-6f);
    stats[kStatNorm] = norm;
    stats[kStatCoef] = finite ? fminf(1.f, q) : q;
    stats[kStatFinite] = finite ? 1.f : 0.f;
    if (!finite) stats[kStatSkipped] += 1.f;
  }
}

// In-place g *= coef over the same descriptors (standalone clip_grad_norm_).
__global__ void grad_scale_kernel(const ChunkDesc* __restrict__ chunks, int nchunks,
                                  const float* __restrict__ stats) {
  const float coef = stats[kStatCoef];
  if (coef == 1.f) return;  // x * 1 == x: nothing to rewrite
  constexpr int V = 4;
  for (int ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    ChunkDesc c = chunks[ci];
    void* gp = const_cast<void*>(c.g);
    const int64_t nv = c.n / V;
    for (int64_t iv = threadIdx.x; iv < nv; iv += blockDim.x) {
      const int64_t idx = c.offset + iv * V;
      float g[V];
      if (c.is_bf16) vload_f32<V>(reinterpret_cast<const bf16*>(gp) + idx, g);
      else vload_f32<V>(reinterpret_cast<const float*>(gp) + idx, g);
#pragma unroll
      for (int k = 0; k < V; ++k) g[k] *= coef;
      if (c.is_bf16) vstore_f32<V>(reinterpret_cast<bf16*>(gp) + idx, g);
      else vstore_f32<V>(reinterpret_cast<float*>(gp) + idx, g);
    }
    for (int64_t i = nv * V + threadIdx.x; i < c.n; i += blockDim.x) {
      const int64_t idx = c.offset + i;
      if (c.is_bf16) {
        bf16* q = reinterpret_cast<bf16*>(gp) + idx;
        *q = f2bf(bf2f(*q) * coef);
      } else {
        reinterpret_cast<float*>(gp)[idx] *= coef;
      }
    }
  }
}

const ChunkDesc* checked_desc(const torch::Tensor& desc, int64_t nchunks) {
  TORCH_CHECK(desc.is_cuda() && desc.scalar_type() == torch::kUInt8 && desc.is_contiguous());
  TORCH_CHECK(nchunks >= 0 && desc.numel() == nchunks * (int64_t)sizeof(ChunkDesc),
              "descriptor table does not hold nchunks entries");
  return reinterpret_cast<const ChunkDesc*>(desc.data_ptr());
}

float* checked_stats(const torch::Tensor& stats) {
  TORCH_CHECK(stats.is_cuda() && stats.scalar_type() == torch::kFloat32 &&
                  stats.is_contiguous() && stats.numel() >= kStatsLen,
              "clip stats: need a contiguous fp32 device tensor of 4 elements");
  return stats.data_ptr<float>();
}

}  // namespace

// Build the chunk-descriptor buffer ONCE (device uint8 tensor). Pointers are
// stable across steps, so the graph-capturable adam_apply path needs no
// per-step host work at all.
std::vector<torch::Tensor> adam_prepare(std::vector<torch::Tensor> ps,
                                        std::vector<torch::Tensor> gs,
                                        std::vector<torch::Tensor> ms,
                                        std::vector<torch::Tensor> vs,
                                        std::vector<c10::optional<torch::Tensor>> masters) {
  std::vector<ChunkDesc> chunks;
  chunks.reserve(512);
  for (size_t t = 0; t < ps.size(); ++t) {
    auto& p = ps[t];
    TORCH_CHECK(p.is_cuda() && p.is_contiguous());
    const bool is_bf16 = p.scalar_type() == torch::kBFloat16;
    float* master = masters[t].has_value() ? masters[t]->data_ptr<float>() : nullptr;
    const int64_t n = p.numel();
    for (int64_t off = 0; off < n; off += kChunkSize) {
      chunks.push_back(ChunkDesc{gs[t].data_ptr(), p.data_ptr(), ms[t].data_ptr<float>(),
                                 vs[t].data_ptr<float>(), master, off,
                                 std::min<int64_t>(kChunkSize, n - off), is_bf16 ? 1 : 0});
    }
  }
  auto host = torch::from_blob(chunks.data(), {(int64_t)(chunks.size() * sizeof(ChunkDesc))},
                               torch::TensorOptions().dtype(torch::kUInt8));
  auto dev = host.to(ps[0].device());
  auto nchunks = torch::tensor({(int64_t)chunks.size()});
  return {dev, nchunks};
}

// Graph-capturable update: lr and step live in device tensors; step is
// incremented on-device first (so a replayed graph advances bias correction).
void adam_apply(torch::Tensor desc, int64_t nchunks, torch::Tensor lr_dev,
                torch::Tensor step_dev, double b1, double b2, double eps, double wd) {
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(incr_kernel, dim3(1), dim3(1), 0, stream, step_dev.data_ptr<int>());
  const int grid = std::min<int>((int)nchunks, 2048);
  hipLaunchKernelGGL(adam_kernel_dev<false>, dim3(grid), dim3(256), 0, stream,
                     reinterpret_cast<const ChunkDesc*>(desc.data_ptr()), (int)nchunks,
                     lr_dev.data_ptr<float>(), step_dev.data_ptr<int>(),
                     static_cast<const float*>(nullptr), (float)b1, (float)b2,
                     1.f - (float)b1, 1.f - (float)b2, (float)eps, (float)wd);
}

void adam_step(std::vector<torch::Tensor> ps, std::vector<torch::Tensor> gs,
               std::vector<torch::Tensor> ms, std::vector<torch::Tensor> vs,
               std::vector<c10::optional<torch::Tensor>> masters, double lr, double b1,
               double b2, double eps, double wd, int64_t step) {
  TORCH_CHECK(ps.size() == gs.size() && ps.size() == ms.size() && ps.size() == vs.size());
  const float bc1 = 1.f - powf((float)b1, (float)step);
  const float bc2 = 1.f - powf((float)b2, (float)step);
  auto stream = at::hip::getCurrentHIPStream();

  std::vector<ChunkDesc> chunks;
  chunks.reserve(512);
  for (size_t t = 0; t < ps.size(); ++t) {
    auto& p = ps[t];
    TORCH_CHECK(p.is_cuda() && p.is_contiguous(), "adam: params must be contiguous cuda");
    TORCH_CHECK(gs[t].is_contiguous() && ms[t].is_contiguous() && vs[t].is_contiguous());
    const bool is_bf16 = p.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(is_bf16 || p.scalar_type() == torch::kFloat32);
    float* master = nullptr;
    if (masters[t].has_value()) master = masters[t]->data_ptr<float>();
    const int64_t n = p.numel();
    for (int64_t off = 0; off < n; off += kChunkSize) {
      chunks.push_back(ChunkDesc{gs[t].data_ptr(), p.data_ptr(), ms[t].data_ptr<float>(),
                                 vs[t].data_ptr<float>(), master, off,
                                 std::min<int64_t>(kChunkSize, n - off), is_bf16 ? 1 : 0});
    }
  }
  // ship descriptors to device in batches
  auto opts = torch::TensorOptions().dtype(torch::kUInt8).device(ps[0].device());
  for (size_t start = 0; start < chunks.size(); start += kMaxChunks) {
    const int nb = (int)std::min<size_t>(kMaxChunks, chunks.size() - start);
    auto host = torch::from_blob(chunks.data() + start, {(int64_t)(nb * sizeof(ChunkDesc))},
                                 torch::TensorOptions().dtype(torch::kUInt8));
    // blocking H2D copy (pageable source); freed buffers are stream-ordered
    // by the caching allocator so the kernel may still read `dev` safely
    auto dev = host.to(opts.device());
    const int grid = std::min(nb, 2048);
    hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(256), 0, stream,
                       reinterpret_cast<const ChunkDesc*>(dev.data_ptr()), nb, (float)lr,
                       (float)b1, (float)b2, (float)eps, (float)wd, bc1, bc2);
    // keep `dev` alive until kernel completion: record it on the stream
    (void)dev;
  }
}

// ---- global-norm clipping entry points --------------------------------------

// Descriptors over a bare gradient list (clip_grad_norm_ without an optimizer):
// only g/offset/n/is_bf16 are filled, which is all the norm and scale kernels read.
std::vector<torch::Tensor> grad_desc_prepare(std::vector<torch::Tensor> gs) {
  TORCH_CHECK(!gs.empty(), "grad_desc_prepare: empty gradient list");
  std::vector<ChunkDesc> chunks;
  chunks.reserve(512);
  for (auto& g : gs) {
    TORCH_CHECK(g.is_cuda() && g.is_contiguous(), "clip: grads must be contiguous cuda");
    const bool is_bf16 = g.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(is_bf16 || g.scalar_type() == torch::kFloat32, "clip: grads must be bf16 or fp32");
    // the kernels use 16-B fp32 / 8-B bf16 accesses
    TORCH_CHECK(reinterpret_cast<uintptr_t>(g.data_ptr()) % (is_bf16 ? 8 : 16) == 0,
                "clip: gradient storage is not vector-aligned");
    const int64_t n = g.numel();
    for (int64_t off = 0; off < n; off += kChunkSize) {
      chunks.push_back(ChunkDesc{g.data_ptr(), nullptr, nullptr, nullptr, nullptr, off,
                                 std::min<int64_t>(kChunkSize, n - off), is_bf16 ? 1 : 0});
    }
  }
  auto host = torch::from_blob(chunks.data(), {(int64_t)(chunks.size() * sizeof(ChunkDesc))},
                               torch::TensorOptions().dtype(torch::kUInt8));
  auto dev = host.to(gs[0].device());
  auto nchunks = torch::tensor({(int64_t)chunks.size()});
  return {dev, nchunks};
}

// Stage 1 for one descriptor table: partials[offset + ci] = sum g^2 of chunk ci.
void grad_sqnorm(torch::Tensor desc, int64_t nchunks, torch::Tensor partials, int64_t offset) {
  const ChunkDesc* d = checked_desc(desc, nchunks);
  TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == torch::kFloat32 &&
              partials.is_contiguous());
  TORCH_CHECK(offset >= 0 && offset + nchunks <= partials.numel(),
              "grad_sqnorm: partials buffer too small");
  if (nchunks == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  const int grid = std::min<int>((int)nchunks, 2048);
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(grid), dim3(kNormThreads), 0, stream, d,
                     (int)nchunks, partials.data_ptr<float>() + offset);
}

// Stage 2 over the partials of every group: writes norm / coef / finite / skipped.
void clip_finalize(torch::Tensor partials, torch::Tensor stats, double max_norm) {
  TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == torch::kFloat32 &&
              partials.is_contiguous());
  TORCH_CHECK(partials.numel() < (int64_t)1 << 31);
  float* st = checked_stats(stats);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(kFinalThreads), 0, stream,
                     partials.data_ptr<float>(), (int)partials.numel(), (float)max_norm, st);
}

// adam_apply with the clip decision read from `stats` on the device.
void adam_apply_clipped(torch::Tensor desc, int64_t nchunks, torch::Tensor lr_dev,
                        torch::Tensor step_dev, torch::Tensor stats, double b1, double b2,
                        double eps, double wd) {
  const ChunkDesc* d = checked_desc(desc, nchunks);
  const float* st = checked_stats(stats);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(incr_if_finite_kernel, dim3(1), dim3(1), 0, stream,
                     step_dev.data_ptr<int>(), st);
  if (nchunks == 0) return;
  const int grid = std::min<int>((int)nchunks, 2048);
  hipLaunchKernelGGL(adam_kernel_dev<true>, dim3(grid), dim3(256), 0, stream, d, (int)nchunks,
                     lr_dev.data_ptr<float>(), step_dev.data_ptr<int>(), st, (float)b1,
                     (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), (float)eps, (float)wd);
}

// g *= stats[coef] in place over a descriptor table.
void grad_scale(torch::Tensor desc, int64_t nchunks, torch::Tensor stats) {
  const ChunkDesc* d = checked_desc(desc, nchunks);
  const float* st = checked_stats(stats);
  if (nchunks == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  const int grid = std::min<int>((int)nchunks, 2048);
  hipLaunchKernelGGL(grad_scale_kernel, dim3(grid), dim3(256), 0, stream, d, (int)nchunks, st);
}
