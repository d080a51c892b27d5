// Shared helpers for jimm_amd CDNA4 (gfx950) kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cmath>

#define WAVE 64  // CDNA wavefront width (not 32!)

#define HIP_CHECK(expr)                                                     \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    if (_e != hipSuccess) {                                                 \
      TORCH_CHECK(false, "HIP error: ", hipGetErrorString(_e), " at ",      \
                  __FILE__, ":", __LINE__);                                 \
    }                                                                       \
  } while (0)

// ---- vector types ----------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef __hip_bfloat16 bf16;

__device__ __forceinline__ float bf2f(bf16 x) { return __bfloat162float(x); }
__device__ __forceinline__ bf16 f2bf(float x) { return __float2bfloat16(x); }

// raw-bits helpers for packed bf16 handled as short
__device__ __forceinline__ float bfs2f(short s) {
  unsigned int u = ((unsigned int)(unsigned short)s) << 16;
  return __uint_as_float(u);
}
__device__ __forceinline__ short f2bfs(float f) {
  bf16 h = __float2bfloat16(f);
  return *reinterpret_cast<short*>(&h);
}

// ---- wave reductions -------------------------------------------------------
__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
  return v;
}

// ---- activations (shared fwd/bwd definitions) ------------------------------
// act codes: 0 = none, 1 = exact erf gelu, 2 = tanh gelu, 3 = quickgelu
#define ACT_NONE 0
#define ACT_GELU 1
#define ACT_GELU_TANH 2
#define ACT_QUICKGELU 3

// Hardware reciprocal (one v_rcp_f32, 1 ulp). `1.0f / x` and __frcp_rn(x)
// both compile to the IEEE division sequence (2 v_div_scale, v_rcp, an fma
// chain, v_div_fmas, v_div_fixup: ~10 VALU per element), which a GEMM
// epilogue cannot afford and a bf16/fp16 result cannot see.
__device__ __forceinline__ float fast_rcpf(float x) { return __builtin_amdgcn_rcpf(x); }

// Fast erfc tail (Abramowitz-Stegun 7.1.26): for ax >= 0 and
// ex = exp(-ax^2), erfc(ax) ~= t*p(t)*ex with t = 1/(1 + 0.3275911 ax).
// The formula itself is good to 1.5e-7 (1.4e-7 in fp64 over [-6, 6]). In
// fp32 the rounding of the Horner chain and of the final 1 - q dominates:
// an fp32 simulation over 3e6 points gives 5.8e-7 with a correctly rounded
// reciprocal and exp, and 8.4e-7 with both off by a whole ulp in the worst
// direction (t*p(t) has slope <= 3.5 in t, so 1 ulp of t <= 1 moves the
// result by at most 2.1e-7). Bound: |err| <= 1e-6 on erf, against 2^-9 for
// a bf16 and 2^-12 for an fp16 result near 1. 7 VALU + 1 v_rcp_f32; the
// caller supplies the exp.
__device__ __forceinline__ float fast_erfc_tail(float ax, float ex) {
  const float t = fast_rcpf(fmaf(0.3275911f, ax, 1.0f));
  float p = 1.061405429f;
  p = fmaf(p, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  return p * t * ex;
}

// erf(x), |err| <= 1e-6 (see fast_erfc_tail): ~12 VALU + 1 v_rcp + 1 v_exp
// vs libm erff's branchy polynomial, which measured ~75 lane-cycles/element
// as a GEMM epilogue.
__device__ __forceinline__ float fast_erff(float x) {
  const float ax = fabsf(x);
  return copysignf(1.0f - fast_erfc_tail(ax, __expf(-ax * ax)), x);
}

__device__ __forceinline__ float fast_tanhf(float x) {
  // tanh(x) = 1 - 2/(exp(2x)+1); clamp avoids exp overflow (|x|>10 -> +-1)
  const float cx = fminf(fmaxf(x, -10.0f), 10.0f);
  return 1.0f - 2.0f * fast_rcpf(__expf(2.0f * cx) + 1.0f);
}

// act(x) and act'(x) from shared sub-expressions: one v_exp_f32 and one
// v_rcp_f32 per element for every activation. act_fwd and act_grad below
// are this function with one output dropped (the compiler removes the dead
// half), so the three always agree and a forward GEMM that also saves the
// derivative returns bitwise the same y as one that does not.
//   erf-GELU: x*Phi(x); derivative Phi(x) + x*phi(x). The erfc tail's
//     exp(-(x/sqrt2)^2) IS the pdf's exp(-x^2/2), so the derivative costs
//     two more operations than the forward.
//   tanh-GELU and QuickGELU: the derivative reuses the tanh / sigmoid.
__device__ __forceinline__ float act_fwd_grad(float x, int act, float* g) {
  switch (act) {
    case ACT_GELU: {
      const float u = x * 0.70710678118654752440f;
      const float au = fabsf(u);
      const float ex = __expf(-au * au);  // exp(-x^2/2)
      const float s = 1.0f + copysignf(1.0f - fast_erfc_tail(au, ex), u);  // 2*Phi(x)
      *g = fmaf(x, 0.3989422804014327f * ex, 0.5f * s);
      return 0.5f * x * s;
    }
    case ACT_GELU_TANH: {
      const float x2 = x * x;
      const float x3 = x2 * x;
      const float t = fast_tanhf(0.7978845608028654f * (x + 0.044715f * x3));
      const float dinner = 0.7978845608028654f * (1.0f + 3.0f * 0.044715f * x2);
      *g = 0.5f * (1.0f + t) + 0.5f * x * (1.0f - t * t) * dinner;
      return 0.5f * x * (1.0f + t);
    }
    case ACT_QUICKGELU: {
      const float s = fast_rcpf(1.0f + __expf(-1.702f * x));
      *g = s + 1.702f * x * s * (1.0f - s);
      return x * s;
    }
    default:
      *g = 1.0f;
      return x;
  }
}

__device__ __forceinline__ float act_fwd(float x, int act) {
  float g;
  return act_fwd_grad(x, act, &g);
}

__device__ __forceinline__ float act_grad(float x, int act) {
  float g;
  act_fwd_grad(x, act, &g);
  return g;
}

// e4m3 (OCP) converts on the hardware v_cvt_pk_fp8_f32 pipe. The HIP
// library __hip_cvt_float_to_fp8 is a ~50-instruction software emulation
// (measured +77 us on a (73856,1024) LayerNorm); the packed builtin is one
// VALU op per 2 elements. Saturate-to-finite by clamping to +-448 first
// (NaN clamps to 448 via IEEE minNum/maxNum; inputs are never NaN here).
__device__ __forceinline__ unsigned short cvt2_e4m3(float a, float b) {
  a = fminf(fmaxf(a, -448.f), 448.f);
  b = fminf(fmaxf(b, -448.f), 448.f);
  return (unsigned short)(__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffff);
}

__device__ __forceinline__ unsigned char cvt_e4m3(float a) {
  return (unsigned char)(cvt2_e4m3(a, 0.f) & 0xff);
}

// ---- counter-based dropout (ops/philox_dropout.py holds the definition) -----------
// Philox4x32, 10 rounds, standard constants: 20 v_mul_lo/v_mul_hi pairs and
// 20 xors per call, no state. Element (m, n) of a rows x cols tensor reads
// counter {m >> 1, (n >> 6) * 16 + (n & 15), site, step}, key {seed lo, seed
// hi}, word (n >> 4) & 3, low half for even m, high half for odd m; so one
// call serves rows {2i, 2i+1} x columns {c, c+16, c+32, c+48} of a 64-group.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                              unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// What a dropout kernel needs beside its data: the device {seed, step} pair
// (read on the device, so a captured graph never bakes the values in), the
// site, the keep threshold t = round(p * 65536) and s = 65536 / (65536 - t).
struct drop_args {
  const long long* rng;
  unsigned site;
  unsigned thresh;
  float scale;
};

// {seed, step} as the key and the last counter word (wave-uniform; load once
// per kernel, outside the element loops).
struct drop_key {
  unsigned k0, k1, step;
};

__device__ __forceinline__ drop_key load_drop_key(const drop_args& d) {
  const unsigned long long seed = (unsigned long long)d.rng[0];
  return {(unsigned)seed, (unsigned)(seed >> 32), (unsigned)d.rng[1]};
}

// The eight 0-or-s multipliers of one Philox call: dm[half][word] for rows
// {2 * mpair + half} and columns {64 * (cgroup >> 4) + 16 * word + (cgroup & 15)}.
__device__ __forceinline__ void drop_mults(const drop_args& d, const drop_key& k, unsigned mpair,
                                           unsigned cgroup, float (&dm)[2][4]) {
  unsigned w[4];
  philox4x32_10(mpair, cgroup, d.site, k.step, k.k0, k.k1, w);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dm[0][i] = (w[i] & 0xffffu) >= d.thresh ? d.scale : 0.f;
    dm[1][i] = (w[i] >> 16) >= d.thresh ? d.scale : 0.f;
  }
}

// Host: t = round(p * 65536), halves up (ops/philox_dropout.py dropout_threshold).
inline unsigned drop_threshold(double p) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout probability must be in [0, 1), got ", p);
  const double t = std::floor(p * 65536.0 + 0.5);
  return t > 65535.0 ? 65535u : (unsigned)t;
}

// Host: kernel arguments of a dropout with threshold t > 0 on x's device.
inline drop_args make_drop_args(unsigned t, const c10::optional<torch::Tensor>& rng,
                                int64_t site, const torch::Tensor& x) {
  TORCH_CHECK(rng.has_value(), "dropout with p > 0 needs the {seed, step} tensor");
  TORCH_CHECK(rng->is_cuda() && rng->device() == x.device() &&
                  rng->scalar_type() == torch::kInt64 && rng->numel() == 2 &&
                  rng->is_contiguous(),
              "dropout rng must be a contiguous int64[2] tensor on the input's device");
  TORCH_CHECK(site >= 0 && site <= 0xffffffffLL, "dropout site must fit 32 bits, got ", site);
  return {reinterpret_cast<const long long*>(rng->data_ptr()), (unsigned)site, t,
          (float)(65536.0 / (65536.0 - (double)t))};
}

// ---- vectorized load/store helpers (G13: hipcc does not auto-vectorize
// bf16 loads; 8-16 B per lane is the coalescing sweet spot) ----------------
template <int V, typename T>
__device__ __forceinline__ void vload_f32(const T* p, float (&o)[V]) {
  if constexpr (sizeof(T) == 2) {
    typedef short vt __attribute__((ext_vector_type(V)));
    vt v = *reinterpret_cast<const vt*>(p);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = bfs2f((short)v[j]);
  } else {
    typedef float vt __attribute__((ext_vector_type(V)));
    vt v = *reinterpret_cast<const vt*>(p);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = v[j];
  }
}

template <int V, typename T>
__device__ __forceinline__ void vstore_f32(T* p, const float (&in)[V]) {
  if constexpr (sizeof(T) == 2) {
    typedef short vt __attribute__((ext_vector_type(V)));
    vt v;
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = f2bfs(in[j]);
    *reinterpret_cast<vt*>(p) = v;
  } else {
    typedef float vt __attribute__((ext_vector_type(V)));
    vt v;
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = in[j];
    *reinterpret_cast<vt*>(p) = v;
  }
}
