// Shared pieces of the MFMA kernels (GEMMs and attention): device primitives
// that several kernels use unchanged, the fused GEMM epilogue, and the host
// helpers that pick a kernel instantiation and launch it.
#pragma once

#include <string>
#include <type_traits>

#include "common.h"

#define MFMA16(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B, C, 0, 0, 0)

// ---- device primitives -----------------------------------------------------

// s_barrier alone: no s_waitcnt in front of it (unlike __syncthreads()), so
// counted vmcnt waits keep staged tiles in flight across the barrier.
__device__ __forceinline__ void raw_barrier() {
  asm volatile("s_barrier" ::: "memory");
}

// 16-byte global -> LDS copy (global_load_lds): lane l's 16 B land at
// lds_dst + l*16 of the wave's base, so lds_dst is wave-linear and any image
// permutation goes on the per-lane SOURCE address.
__device__ __forceinline__ void glds16(const bf16* g, char* lds_dst) {
  // C-style casts perform the addrspace conversion (generic->AS1/AS3);
  // reinterpret_cast refuses (same idiom as CK's c_style_pointer_cast)
  typedef const __attribute__((address_space(1))) unsigned int* gp_t;
  typedef __attribute__((address_space(3))) unsigned int* lp_t;
  __builtin_amdgcn_global_load_lds((gp_t)(const void*)g, (lp_t)(void*)lds_dst, 16, 0, 0);
}

// XCD-aware bijective remap of the linear workgroup id (guide T1): the
// hardware deals workgroups round-robin over the 8 XCDs, so XCD x gets the
// contiguous run of tiles starting at its share of nwg — neighbouring tiles
// share an L2.
__device__ __forceinline__ int xcd_remap(int wg, int nwg) {
  const int q = nwg / 8, r = nwg % 8;
  const int xcd = wg % 8, idx = wg / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// Guarded 8-element load for head dims beyond 64: kernels are templated on
// the PADDED head dim DP in {64, 96, 128} (d-fragments need multiples of 32)
// and the runtime Dr (72, 80 pad to 96) guards ragged chunks — 8-element
// chunks are all-in or all-out since every supported D is a multiple of 8.
template <int DP>
__device__ __forceinline__ bf16x8 ld8g(const bf16* p, int off, int Dr) {
  if (DP == 64 || off + 8 <= Dr) return *reinterpret_cast<const bf16x8*>(p + off);
  return bf16x8{};
}

// Block-format image for transposed fragment reads (the gemm_tn8p.hip
// recipe): a [64 q][ND d] tile stored as [q-half (q>>5)][d16 (d>>4)]
// [8 q-quads, evens first][4][16] — written from row-major registers with
// ds_write_b128 (two vector writes per 16-d chunk instead of 16 scalar
// transpose stores, which were 8-way bank-conflicted), and read as MFMA
// B-fragments with batched ds_read_b64_tr_b16 at per-lane address
// base + lane*8 B (mapping verified by ext.tr16_probe).
template <int ND>
__device__ __forceinline__ int boff(int q, int d) {
  const int qp = (q >> 2) & 7;
  const int qpos = (qp & 1) * 4 + (qp >> 1);
  return (q >> 5) * (32 * ND) + (d >> 4) * 512 + qpos * 64 + (q & 3) * 16 + (d & 15);
}

typedef const __attribute__((address_space(3))) char* lds_cp;

// 4 B-fragments (dt, dt+1, dt+2, dt+3) of one 32-contraction step from a
// block image: 8 tr reads + lgkmcnt(0) in one asm (guide §5.7 form i).
__device__ __forceinline__ void tr_frag_x4(lds_cp base, bf16x8 (&out)[4]) {
  bf16x4 a0l, a0h, a1l, a1h, a2l, a2h, a3l, a3h;
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
      : "v"(base)
      : "memory");
  __builtin_amdgcn_sched_barrier(0);
  out[0] = __builtin_shufflevector(a0l, a0h, 0, 1, 2, 3, 4, 5, 6, 7);
  out[1] = __builtin_shufflevector(a1l, a1h, 0, 1, 2, 3, 4, 5, 6, 7);
  out[2] = __builtin_shufflevector(a2l, a2h, 0, 1, 2, 3, 4, 5, 6, 7);
  out[3] = __builtin_shufflevector(a3l, a3h, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ void tr_frag_x2(lds_cp base, bf16x8 (&out)[2]) {
  bf16x4 a0l, a0h, a1l, a1h;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4 offset:0\n\t"
      "ds_read_b64_tr_b16 %1, %4 offset:512\n\t"
      "ds_read_b64_tr_b16 %2, %4 offset:1024\n\t"
      "ds_read_b64_tr_b16 %3, %4 offset:1536\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(a0l), "=&v"(a0h), "=&v"(a1l), "=&v"(a1h)
      : "v"(base)
      : "memory");
  __builtin_amdgcn_sched_barrier(0);
  out[0] = __builtin_shufflevector(a0l, a0h, 0, 1, 2, 3, 4, 5, 6, 7);
  out[1] = __builtin_shufflevector(a1l, a1h, 0, 1, 2, 3, 4, 5, 6, 7);
}

// The NT = DP/16 B-fragments (4, 6 or 8) of one 32-contraction step.
template <int NT>
__device__ __forceinline__ void tr_frags(lds_cp base, bf16x8 (&out)[NT]) {
  static_assert(NT == 4 || NT == 6 || NT == 8, "head dims 64, 96, 128");
  tr_frag_x4(base, *reinterpret_cast<bf16x8(*)[4]>(&out[0]));
  if constexpr (NT == 6) tr_frag_x2(base + 4096, *reinterpret_cast<bf16x8(*)[2]>(&out[4]));
  if constexpr (NT == 8) tr_frag_x4(base + 4096, *reinterpret_cast<bf16x8(*)[4]>(&out[4]));
}

// The A/B fragment of contraction step `step` (columns 32*step + 8*hi .. +8 of
// one row) from a row-major LDS image with `pitch` shorts per row. step and hi
// are two arguments so that they are added to the pointer one after the
// other: handed over as one summed column, the forward kernels compile to
// different address arithmetic (5 more v_add3_u32, another VGPR count).
__device__ __forceinline__ bf16x8 row_frag(const short* img, int row, int pitch, int step,
                                           int hi) {
  return *reinterpret_cast<const bf16x8*>(img + row * pitch + 32 * step + hi * 8);
}

// ---- attention: (B,H,L,D) views ---------------------------------------------

// Element strides of one (B,H,L,D) view whose innermost dim is contiguous.
// Kernels take one per tensor, next to its pointer (the pointers stay
// separate __restrict__ parameters).
struct hstride {
  int64_t b, h, l;
};

// Row 0 of head bh = b*H + h.
template <typename T>
__device__ __forceinline__ T* head_ptr(T* base, const hstride& s, int64_t bh, int H) {
  return base + (bh / H) * s.b + (bh % H) * s.h;
}

// ---- attention: resident kernels (one workgroup per head) --------------------

// Domain of the resident forward and backward: D = 64, Lq == Lk = L,
// non-causal, RES_LMIN <= L <= RES_LMAX, res_aligned views (host section).
constexpr int RES_LMIN = 81;
constexpr int RES_LMAX = 256;

// Natural-order block image of a [rows][64 d] operand: 32-row blocks of four
// 16-d sub-blocks, rows 32 B apart inside a sub-block. Unlike boff<> the 8
// row-quads keep their order, which is what lets two accumulator tiles serve
// as the next MFMA's fragment (attention_bwd_fused.hip, resident kernel).
__device__ __forceinline__ int noff(int row, int d) {
  return (row >> 5) * 2048 + (d >> 4) * 512 + (row & 31) * 16 + (d & 15);
}

// ---- fused GEMM epilogue ---------------------------------------------------

// What a forward GEMM writes to Z beside Y: nothing, the pre-activation
// (bf16), or the activation derivative act'(vpre) as fp16 (activated GEMMs
// only). The derivative lies in about [-0.17, 1.13], so fp16's 11 bits cost
// no range, and the backward is left with one multiply (GRADM_MUL).
#define SAVE_NONE 0
#define SAVE_PRE 1
#define SAVE_GRAD 2

// dX GEMM of an activated linear with the activation backward fused in:
// GRADM_ACT recomputes act'(z) from the saved bf16 pre-activation,
// GRADM_MUL reads the saved fp16 derivative. res carries either.
#define GRADM_NONE 0
#define GRADM_ACT 1
#define GRADM_MUL 2

// bias[n] as fp32 from an fp32 or a bf16 bias vector (wave-uniform flag; a
// lane needs only the few columns it owns, so callers load these once per
// tile, outside the element loops).
__device__ __forceinline__ float load_bias(const void* bias, int n, int bias_bf16) {
  return bias_bf16 ? bf2f(static_cast<const bf16*>(bias)[n])
                   : static_cast<const float*>(bias)[n];
}

// One accumulator value of an NT GEMM at (m, n), already inside the bounds:
//   vpre = acc (+ bias_n);  Z = vpre (SAVE_PRE) or fp16 act'(vpre) (SAVE_GRAD)
//   Y = act(vpre) (+ res)                      forward
//   Y = vpre * act'(res)                       GRADM_ACT
//   Y = vpre * res (fp16)                      GRADM_MUL
//   Y8 = e4m3(Y * rs8), *tmax = max(*tmax, |Y|)   FP8O: delayed-scaled e4m3
//       copy (consumed by the fp8 dX GEMM); the caller reduces tmax.
// Y is the same bits in every SAVE mode: act_fwd is act_fwd_grad with the
// derivative dropped.
// DROP (forward only): dm is this element's dropout multiplier, 0 or
// s = 1 / keep rate (common.h); it scales act(vpre) before the residual is
// added and the saved derivative, so the backward of the dropout that follows
// an activation is already in Z:
//   Y = dm * bf16(act(vpre)) with an activation, dm * vpre (+ res) without;
//   Z = fp16 dm * act'(vpre) (SAVE_GRAD)
template <int ACT, bool HAS_BIAS, bool HAS_RES, int SAVE, int GRADM = GRADM_NONE,
          bool FP8O = false, bool DROP = false>
__device__ __forceinline__ void gemm_epilogue(float vpre, int m, int n, int N, float bias_n,
                                              const bf16* res, bf16* Y, bf16* Z,
                                              unsigned char* Y8 = nullptr, float rs8 = 1.f,
                                              float* tmax = nullptr, float dm = 1.f) {
  static_assert(SAVE != SAVE_GRAD || ACT != ACT_NONE, "SAVE_GRAD needs an activation");
  static_assert(!DROP || (GRADM == GRADM_NONE && SAVE != SAVE_PRE && !FP8O),
                "dropout epilogue: forward GEMMs that save nothing or the derivative");
  if (HAS_BIAS) vpre += bias_n;
  if (SAVE == SAVE_PRE) Z[(int64_t)m * N + n] = f2bf(vpre);
  float vy;
  if (GRADM == GRADM_ACT) {
    vy = vpre * act_grad(bf2f(res[(int64_t)m * N + n]), ACT);
  } else if (GRADM == GRADM_MUL) {
    vy = vpre * __half2float(reinterpret_cast<const __half*>(res)[(int64_t)m * N + n]);
  } else {
    if (SAVE == SAVE_GRAD) {
      float g;
      vy = act_fwd_grad(vpre, ACT, &g);
      if (DROP) g *= dm;
      reinterpret_cast<__half*>(Z)[(int64_t)m * N + n] = __float2half(g);
    } else {
      vy = act_fwd(vpre, ACT);
    }
    if (DROP) {
      // an activated output is rounded to bf16 BEFORE it is scaled: Y is then
      // bit for bit dropout_fwd of the p = 0 output (one rounding away from
      // s times it, not two), and the fused and the unfused block agree
      if (ACT != ACT_NONE) vy = bf2f(f2bf(vy));
      vy *= dm;
    }
    if (HAS_RES) vy += bf2f(res[(int64_t)m * N + n]);
  }
  Y[(int64_t)m * N + n] = f2bf(vy);
  if (FP8O) {
    *tmax = fmaxf(*tmax, fabsf(vy));
    Y8[(int64_t)m * N + n] = cvt_e4m3(vy * rs8);
  }
}

// bias[n .. n+3] as fp32, n a multiple of 4: one 16-byte fp32 or one 8-byte
// bf16 load (the vector must be 16- resp. 8-byte aligned).
__device__ __forceinline__ void load_bias4(const void* bias, int n, int bias_bf16,
                                           float (&b)[4]) {
  if (bias_bf16) vload_f32<4>(static_cast<const bf16*>(bias) + n, b);
  else vload_f32<4>(static_cast<const float*>(bias) + n, b);
}

// Makes x depend on tok without changing it (no instruction): what is
// computed from x can then neither be hoisted above tok nor be paired with the
// computation of tok.
// The same with nothing to wait for: what consumes x (a packed store) is cut
// off from what computed it.
__device__ __forceinline__ void opaque(float& x) { asm("" : "+v"(x)); }
__device__ __forceinline__ void opaque(unsigned int& x) { asm("" : "+v"(x)); }
__device__ __forceinline__ void after(float& x, float tok) { asm("" : "+v"(x) : "v"(tok)); }
__device__ __forceinline__ void after(float& x, unsigned int tok) {
  asm("" : "+v"(x) : "v"(tok));
}

// gemm_epilogue for the 4 consecutive columns n .. n+3 (n a multiple of 4) of
// row m that a lane of the column-permuted 8-phase kernel holds (gemm8p.hip):
// every stream is one access (8 bytes of bf16 or fp16, 4 bytes of e4m3)
// instead of four. Y, Z and res must be 8-byte aligned, Y8 4-byte, and N a
// multiple of 4. No dropout form: its Philox words are tied to the 16-apart
// columns of the unpermuted kernel.
// Per element it is gemm_epilogue's arithmetic, and it has to compile to
// gemm_epilogue's instructions as well. Four independent copies of the
// activation code in a row get packed in pairs (v_pk_mul_f32, v_pk_add_f32)
// BEFORE multiplies and adds are contracted, which leaves fewer fmas than the
// per-element code has (tanh-GELU: x2 * c + 1 and 1 - t * t stay unfused) and
// replaces the fp16 derivative's single rounding (v_fma_mixlo_f16) by a
// packed fma and a conversion: other rounding points, other bits. So with an
// activation the elements are chained and closed off: element j's inputs come
// `after` element j - 1's results, and its results are `opaque` to the packed
// stores, so the vectoriser finds no group of like operations to start from,
// across the elements. erf-GELU and QuickGELU then compile to gemm_epilogue's
// instructions per element (same bits). tanh-GELU does not quite: the
// compiler also pairs two like operations INSIDE one element (1 - 2r with
// 1 + c*x^2) and leaves them unfused, here in every kernel, under
// gemm_epilogue in some; those results agree to rounding, not bit for bit.
// Without an activation there is nothing to contract (adds, or one multiply)
// and the packing is left alone.
template <int ACT, bool HAS_BIAS, bool HAS_RES, int SAVE, int GRADM = GRADM_NONE,
          bool FP8O = false>
__device__ __forceinline__ void gemm_epilogue4(const float (&acc4)[4], int m, int n, int N,
                                               const float (&bias4)[4], const bf16* res, bf16* Y,
                                               bf16* Z, unsigned char* Y8 = nullptr,
                                               float rs8 = 1.f, float* tmax = nullptr) {
  static_assert(SAVE != SAVE_GRAD || ACT != ACT_NONE, "SAVE_GRAD needs an activation");
  typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
  constexpr bool READS = GRADM != GRADM_NONE || HAS_RES;  // res holds a residual, z or g
  constexpr bool CHAIN = ACT != ACT_NONE;
  const int64_t at = (int64_t)m * N + n;
  float vpre[4], vy[4], in4[4] = {};
  u16x4 g4 = {};
  if (GRADM == GRADM_MUL) {
    const u16x4 h4 = *reinterpret_cast<const u16x4*>(res + at);
#pragma unroll
    for (int j = 0; j < 4; ++j) in4[j] = __half2float(__ushort_as_half(h4[j]));
  } else if (READS) {
    vload_f32<4>(res + at, in4);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    vpre[j] = HAS_BIAS ? acc4[j] + bias4[j] : acc4[j];
    if (CHAIN && j > 0) {
      after(vpre[j], vy[j - 1]);
      if (READS) after(in4[j], vy[j - 1]);
      if (SAVE == SAVE_GRAD) after(vpre[j], (unsigned int)g4[j - 1]);
    }
    if (GRADM == GRADM_ACT) {
      vy[j] = vpre[j] * act_grad(in4[j], ACT);
    } else if (GRADM == GRADM_MUL) {
      vy[j] = vpre[j] * in4[j];
    } else {
      if (SAVE == SAVE_GRAD) {
        float g;
        vy[j] = act_fwd_grad(vpre[j], ACT, &g);
        unsigned int gb = __half_as_ushort(__float2half(g));
        if (CHAIN) opaque(gb);
        g4[j] = (unsigned short)gb;
      } else {
        vy[j] = act_fwd(vpre[j], ACT);
      }
      if (HAS_RES) vy[j] += in4[j];
    }
    if (CHAIN) opaque(vy[j]);
  }
  if (SAVE == SAVE_PRE) vstore_f32<4>(Z + at, vpre);
  if (SAVE == SAVE_GRAD) *reinterpret_cast<u16x4*>(Z + at) = g4;
  vstore_f32<4>(Y + at, vy);
  if (FP8O) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *tmax = fmaxf(*tmax, fabsf(vy[j]));
    // cvt_e4m3(a) is the low byte of cvt2_e4m3(a, .), b's byte is the next one
    *reinterpret_cast<unsigned int*>(Y8 + at) =
        (unsigned int)cvt2_e4m3(vy[0] * rs8, vy[1] * rs8) |
        ((unsigned int)cvt2_e4m3(vy[2] * rs8, vy[3] * rs8) << 16);
  }
}

// ---- host: kernel selection and launch -------------------------------------

// activation name -> ACT_* code ("" = none); throws on an unknown name
// (elementwise.hip)
int act_code(const std::string& act);

// Run-time values -> template arguments. with_int calls f with the
// std::integral_constant<int, V> whose V equals v and throws "bad <what> <v>"
// when none does; with_act (ACT_*) and with_save (SAVE_*) are the two fixed
// lists. with_flags calls f with one std::true_type / std::false_type per
// bool, in order. Read them back with decltype(c)::value.
template <int... Vs, typename F>
void with_int(int v, const char* what, F&& f) {
  const bool found = ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
  TORCH_CHECK(found, "bad ", what, " ", v);
}

template <typename F>
void with_act(int act, F&& f) {
  with_int<ACT_NONE, ACT_GELU, ACT_GELU_TANH, ACT_QUICKGELU>(act, "activation code", f);
}

template <typename F>
void with_save(int save, F&& f) {
  with_int<SAVE_NONE, SAVE_PRE, SAVE_GRAD>(save, "save mode", f);
}

template <typename F>
void with_flags(F&& f) {
  f();
}
template <typename F, typename... Rest>
void with_flags(F&& f, bool b, Rest... rest) {
  if (b) with_flags([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
  else with_flags([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

// Launches Kernel with `shmem` bytes of dynamic LDS. Before its first launch
// each kernel gets its dynamic-LDS limit raised to `shmem_limit` (>= every
// shmem it will be launched with); a refusal surfaces here instead of as a
// failed launch later.
template <auto Kernel, typename... Args>
void launch_lds(dim3 grid, dim3 block, size_t shmem, size_t shmem_limit, hipStream_t stream,
                Args... args) {
  static const bool raised = [&] {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)shmem_limit));
    return true;
  }();
  (void)raised;
  hipLaunchKernelGGL(Kernel, grid, block, shmem, stream, args...);
}

// ---- host: attention arguments ----------------------------------------------

inline hstride hstrides(const torch::Tensor& t) {
  return {t.stride(0), t.stride(1), t.stride(2)};
}

inline bf16* bf16_ptr(const torch::Tensor& t) {
  return reinterpret_cast<bf16*>(t.data_ptr());
}

// The resident attention kernels load 16 and store 8 bytes at a time: every
// base must be 16-byte aligned and every stride a multiple of 8 elements
// (true of every view the model passes; anything else stays on a tiled path).
inline bool res_aligned(std::initializer_list<const torch::Tensor*> ts) {
  bool ok = true;
  for (const torch::Tensor* t : ts)
    ok = ok && reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0 && t->stride(0) % 8 == 0 &&
         t->stride(1) % 8 == 0 && t->stride(2) % 8 == 0;
  return ok;
}

struct named_tensor {
  const char* name;
  const torch::Tensor& t;
};

// Argument checks of attn_fwd and attn_bwd_fused. Every tensor is a CUDA
// bf16 (B,H,L,D) view with a contiguous innermost dim and a supported head
// dim; q_like (q first: q, o, dO, dq) share q's shape, k_like (k first: k, v,
// dk, dv) share k's, and k agrees with q in B, H and D. lse, where given, is
// contiguous fp32 with B*H*Lq elements.
inline void check_attn_args(const char* op, std::initializer_list<named_tensor> q_like,
                            std::initializer_list<named_tensor> k_like,
                            const torch::Tensor* lse = nullptr) {
  const torch::Tensor& q = q_like.begin()->t;
  const torch::Tensor& k = k_like.begin()->t;
  for (const auto* list : {&q_like, &k_like}) {
    const torch::Tensor& first = list->begin()->t;
    for (const named_tensor& n : *list) {
      TORCH_CHECK(n.t.is_cuda(), op, ": ", n.name, " must be a CUDA tensor");
      TORCH_CHECK(n.t.scalar_type() == torch::kBFloat16, op, ": ", n.name,
                  " must be bf16, got ", n.t.scalar_type());
      TORCH_CHECK(n.t.dim() == 4, op, ": ", n.name, " must be (B,H,L,D), got ", n.t.dim(),
                  " dims");
      TORCH_CHECK(n.t.stride(3) == 1, op, ": innermost dim of ", n.name,
                  " must be contiguous");
      TORCH_CHECK(n.t.sizes() == first.sizes(), op, ": ", n.name, " has shape ", n.t.sizes(),
                  ", expected ", list->begin()->name, "'s ", first.sizes());
    }
  }
  const int64_t D = q.size(3);
  TORCH_CHECK(D == 64 || D == 72 || D == 80 || D == 96 || D == 128, op,
              ": head_dim must be one of {64,72,80,96,128}, got ", D);
  TORCH_CHECK(k.size(0) == q.size(0) && k.size(1) == q.size(1) && k.size(3) == D, op,
              ": k has shape ", k.sizes(), ", expected q's B, H and D ", q.sizes());
  if (lse) {
    TORCH_CHECK(lse->is_cuda() && lse->is_contiguous() &&
                    lse->scalar_type() == torch::kFloat32 &&
                    lse->numel() == q.size(0) * q.size(1) * q.size(2),
                op, ": lse must be contiguous fp32 (B,H,Lq)");
  }
}
