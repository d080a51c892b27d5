// K5 — flash-style attention forward for CDNA4 (gfx950), bf16, head_dim 64.
//
// Covers every attention in the model zoo: self-attention
// L in {50..1024} (ViT/CLIP/SigLIP towers, all with head_dim 64 since
// heads = width/64 — clip.py:60), causal masking for the CLIP text tower
// (clip.py:62), and the MAP head's Lq=1 cross-attention (K9).
//
// Design (one workgroup = 4 waves = 64 q rows; grid = (ceil(Lq/64), B*H)):
//   * "swapped" QK^T: S^T = mfma(A=K_tile, B=Q^T) so each lane's softmax
//     row stats live in-lane + 2 shuffles (no serial-lane softmax — CDNA
//     guide common-mistake #6);
//   * K staged row-major in LDS, V staged TRANSPOSED (V^T) so the PV
//     mfma's B-fragment is a contiguous ds_read_b128;
//   * P routed through a per-wave LDS tile (padded rows, +8 shorts) to
//     re-shape from the S^T C-layout into the PV A-fragment layout;
//   * online softmax with running (m, l) per q row; lse = m + log(l)
//     saved for the backward (recompute) pass.
//
// MFMA: v_mfma_f32_16x16x32_bf16. Fragment layouts (verified on hardware by
// csrc/probe.hip + tests/test_kernels_gpu.py::test_mfma_probe):
//   A[i][k]: lane l holds A[l&15][(l>>4)*8 + j], j=0..7
//   B[k][j]: lane l holds B[(l>>4)*8 + j][l&15]
//   C[i][j]: lane l holds rows (l>>4)*4+r (r=0..3), col l&15

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "mfma.h"

namespace {

typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int QBLK = 64;    // q rows per strip (16 per wave)
// NSTRIP (q strips per workgroup) is a template param: 4 = fewer K/V
// staging passes, 2 waves/SIMD; 2 = 3 waves/SIMD, twice the staging
// (JIMM_AMD_ATTN_NSTRIP selects; default 4)
constexpr int KVBLK = 64;   // keys per LDS tile

// Head dims beyond 64: the kernel is templated on the
// padded head dim DP and loads through ld8g<DP> (mfma.h).
//
// V block image (boff<DP>, mfma.h): [64 key][DP d], written with vector
// ds_write_b128 from the row-major staging registers and read as PV
// B-fragments with tr_frag_x4 / tr_frag_x2 at per-lane address
// base + lane*8 B.

template <bool CAUSAL, int NSTRIP, int DP>
__global__ __launch_bounds__(256) void attn_fwd_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    bf16* __restrict__ o, float* __restrict__ lse, int Lq, int Lk, float scale, int H, int Dr,
    int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
    int64_t v_sb, int64_t v_sh, int64_t v_sl, int64_t o_sb, int64_t o_sh, int64_t o_sl) {
  // (sb, sh, sl) = element strides of the (B,H,L,64) view; innermost dim is
  // contiguous. Covers contiguous BHLD, (B,L,H,64) and fused-qkv (B,L,3,H,64)
  // layouts with no permute copies.
  //
  // Each workgroup covers up to NSTRIP x 64 q rows of one (b,h): K/V tiles
  // are staged ONCE per kv tile for all strips (the 1-strip version staged
  // them once per 64-q workgroup — 4x redundant global traffic at L=197,
  // ~125 of its 213 us bandwidth-bound). T14 split staging + single LDS
  // buffer; each wave keeps NSTRIP online-softmax states.
  constexpr int LDS_PITCH = DP + 8;  // bank-conflict pad for b128 reads
  constexpr int NS = DP / 32;        // d-steps per fragment contraction
  constexpr int NT = DP / 16;        // d-tiles of the output
  // K/V staging double-buffered: tile it+1's write pass runs under tile
  // it's compute into the other buffer; ONE barrier per kv tile
  constexpr int IMGSF = KVBLK * LDS_PITCH + KVBLK * DP;  // per buffer
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* k_lds = reinterpret_cast<short*>(smem);                       // KVBLK rows
  short* vt_lds = k_lds + KVBLK * LDS_PITCH;                           // V block image [KVBLK][DP]
  short* p_lds = reinterpret_cast<short*>(smem) + 2 * IMGSF;           // 4*16 rows

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int lo = lane & 15;   // column index inside a 16-wide fragment
  const int hi = lane >> 4;   // 0..3
  const int64_t bh = blockIdx.y;
  const int64_t b = bh / H, h = bh % H;
  // cyclic strip -> q-tile mapping: strip t covers q tile
  // (blockIdx.x + t*gridDim.x) — balances ragged L (a blocked mapping gives
  // the last workgroup a nearly-empty supertile, e.g. 1 of 256 rows at L=257)
  const int ntq = (Lq + QBLK - 1) / QBLK;

  const bf16* qp = q + b * q_sb + h * q_sh;
  const bf16* kp = k + b * k_sb + h * k_sh;
  const bf16* vp = v + b * v_sb + h * v_sh;
  bf16* op = o + b * o_sb + h * o_sh;

  // ---- load Q fragments for every strip (B-operand of the swapped QK^T) --
  // strip t covers q rows [q_base + t*64, +64); this wave's rows:
  // q0(t) = q_base + t*64 + wave*16; B[d][q] = Q[q0+lo][32*s + hi*8 + j]
  bf16x8_t qb[NSTRIP][NS];
  int nactive = 0;
#pragma unroll
  for (int t = 0; t < NSTRIP; ++t) {
    const int ti = blockIdx.x + t * gridDim.x;
    if (ti < ntq) nactive = t + 1;
    const int qrow = min(min(ti, ntq - 1) * QBLK + wave * 16 + lo, Lq - 1);
#pragma unroll
    for (int s = 0; s < NS; ++s)
      qb[t][s] = ld8g<DP>(qp + (int64_t)qrow * q_sl, 32 * s + hi * 8, Dr);
  }

  short* my_p = p_lds + wave * 16 * LDS_PITCH;

  f32x4_t acc_o[NSTRIP][NT] = {};  // O tiles: rows q = hi*4+r, cols d = 16*dt+lo
  float m_run[NSTRIP], l_run[NSTRIP];
#pragma unroll
  for (int t = 0; t < NSTRIP; ++t) {
    m_run[t] = -INFINITY;
    l_run[t] = 0.f;
  }

  const int ti_max = blockIdx.x + (nactive - 1) * gridDim.x;  // last active tile
  const int kv_end = CAUSAL ? min(Lk, (ti_max + 1) * QBLK) : Lk;

  // T14 staging state
  constexpr int NCG = (DP + 63) / 64;  // 64-wide column groups per row
  const int st_row = tid / 4;
  const int st_c0 = (tid % 4) * 16;
  bf16x8_t kreg[NCG][2], vreg[NCG][2];
  bool st_valid;
  auto load_tile_regs = [&](int kv0) {
    const int key = kv0 + st_row;
    st_valid = key < Lk;
    const int krow = min(key, Lk - 1);
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
      const int c0 = cg * 64 + st_c0;
      if (c0 >= DP) continue;
      kreg[cg][0] = ld8g<DP>(kp + (int64_t)krow * k_sl, c0, Dr);
      kreg[cg][1] = ld8g<DP>(kp + (int64_t)krow * k_sl, c0 + 8, Dr);
      vreg[cg][0] = ld8g<DP>(vp + (int64_t)krow * v_sl, c0, Dr);
      vreg[cg][1] = ld8g<DP>(vp + (int64_t)krow * v_sl, c0 + 8, Dr);
    }
  };
  auto write_tile = [&](int buf) {
    const int bo = buf * IMGSF;
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
      const int c0 = cg * 64 + st_c0;
      if (c0 >= DP) continue;
      const bf16x8_t k0 = st_valid ? kreg[cg][0] : bf16x8_t{};
      const bf16x8_t k1 = st_valid ? kreg[cg][1] : bf16x8_t{};
      const bf16x8_t v0 = st_valid ? vreg[cg][0] : bf16x8_t{};
      const bf16x8_t v1 = st_valid ? vreg[cg][1] : bf16x8_t{};
      *reinterpret_cast<bf16x8_t*>(k_lds + bo + st_row * LDS_PITCH + c0) = k0;
      *reinterpret_cast<bf16x8_t*>(k_lds + bo + st_row * LDS_PITCH + c0 + 8) = k1;
      *reinterpret_cast<bf16x8_t*>(vt_lds + bo + boff<DP>(st_row, c0)) = v0;
      *reinterpret_cast<bf16x8_t*>(vt_lds + bo + boff<DP>(st_row, c0 + 8)) = v1;
    }
  };

  const int ntiles = (kv_end + KVBLK - 1) / KVBLK;
  load_tile_regs(0);
  write_tile(0);
  if (ntiles > 1) load_tile_regs(KVBLK);
  __syncthreads();

  for (int it = 0; it < ntiles; ++it) {
    const int kv0 = it * KVBLK;
    const int sbo = (it & 1) * IMGSF;
    if (it + 1 < ntiles) {
      write_tile((it + 1) & 1);
      if (it + 2 < ntiles) load_tile_regs(kv0 + 2 * KVBLK);
    }
#pragma unroll
    for (int st = 0; st < NSTRIP; ++st) {
      const int ti = blockIdx.x + st * gridDim.x;
      const int q0 = ti * QBLK + wave * 16;
      if (ti >= ntq || q0 >= Lq) continue;
      if (CAUSAL && kv0 >= (ti + 1) * QBLK) continue;  // fully masked strip
      // keys beyond kv_hi are padding (>= Lk) or above this wave-strip's
      // causal diagonal (> q0+15): their sub-tiles are skipped outright —
      // at L=77 causal ~3/4 of the key sub-tiles are pure waste otherwise
      //  — and masked to -inf / P=0 below.
      const int kv_hi = CAUSAL ? min(Lk, q0 + 16) : Lk;
      // ---- S^T = K . Q^T : 4 key tiles x NS d-steps -----------------------
      __builtin_amdgcn_s_setprio(1);
      f32x4_t sc[4] = {};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (kv0 + 16 * t >= kv_hi) continue;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const bf16x8_t ka =
              *reinterpret_cast<const bf16x8_t*>(k_lds + sbo + (16 * t + lo) * LDS_PITCH + 32 * s + hi * 8);
          sc[t] = MFMA16(ka, qb[st][s], sc[t]);
        }
      }
      __builtin_amdgcn_s_setprio(0);

      // ---- masked, scaled scores; per-row (q = lo) online softmax --------
      float sv[16];
      const int q_idx = q0 + lo;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kv0 + 16 * t + hi * 4 + r;
          float x = sc[t][r] * scale;
          if (key >= Lk || (CAUSAL && key > q_idx)) x = -INFINITY;
          sv[4 * t + r] = x;
        }
      }
      float mt = sv[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) mt = fmaxf(mt, sv[i]);
      mt = fmaxf(mt, __shfl_xor(mt, 16, WAVE));
      mt = fmaxf(mt, __shfl_xor(mt, 32, WAVE));

      const float m_new = fmaxf(m_run[st], mt);
      // alpha=0 on the first tile (m_run = -inf) starts O from zero
      const float alpha = (m_new == -INFINITY) ? 0.f : __expf(m_run[st] - m_new);
      m_run[st] = m_new;

      float psum = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = (sv[i] == -INFINITY) ? 0.f : __expf(sv[i] - m_new);
        sv[i] = p;
        psum += p;
      }
      psum += __shfl_xor(psum, 16, WAVE);
      psum += __shfl_xor(psum, 32, WAVE);
      l_run[st] = l_run[st] * alpha + psum;

      // ---- write P (bf16) into this wave's LDS tile: [q=lo][k=16t+4hi+r] -
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        bf16x4 pk;
#pragma unroll
        for (int r = 0; r < 4; ++r) pk[r] = f2bfs(sv[4 * t + r]);
        *reinterpret_cast<bf16x4*>(my_p + lo * LDS_PITCH + 16 * t + hi * 4) = pk;
      }

      // ---- rescale O accumulators (rows q = hi*4+r need alpha of lane q) -
      float alpha_r[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) alpha_r[r] = __shfl(alpha, hi * 4 + r, WAVE);
#pragma unroll
      for (int dt = 0; dt < NT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc_o[st][dt][r] *= alpha_r[r];

      // ---- O += P . V : A = P (from LDS), B = V^T via tr reads -----------
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (kv0 + 32 * s >= kv_hi) continue;  // P = 0 for the whole step
        bf16x8_t vb[NT];
        const lds_cp bbase = (lds_cp)(const void*)(vt_lds + sbo + s * 32 * DP) + lane * 8;
        tr_frag_x4(bbase, *reinterpret_cast<bf16x8_t(*)[4]>(&vb[0]));
        if constexpr (NT == 6) tr_frag_x2(bbase + 4096, *reinterpret_cast<bf16x8_t(*)[2]>(&vb[4]));
        if constexpr (NT == 8) tr_frag_x4(bbase + 4096, *reinterpret_cast<bf16x8_t(*)[4]>(&vb[4]));
        const bf16x8_t pa =
            *reinterpret_cast<const bf16x8_t*>(my_p + lo * LDS_PITCH + 32 * s + hi * 8);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int dt = 0; dt < NT; ++dt) acc_o[st][dt] = MFMA16(pa, vb[dt], acc_o[st][dt]);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    // double-buffered: ONE barrier publishes tile it+1 and retires it
    __syncthreads();
  }

  // ---- epilogue: O /= l, store O and lse ----------------------------------
#pragma unroll
  for (int st = 0; st < NSTRIP; ++st) {
    const int ti = blockIdx.x + st * gridDim.x;
    const int q0 = ti * QBLK + wave * 16;
    if (ti >= ntq || q0 >= Lq) continue;
    const float invl = (l_run[st] > 0.f) ? 1.f / l_run[st] : 0.f;
    float invl_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) invl_r[r] = __shfl(invl, hi * 4 + r, WAVE);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = q0 + hi * 4 + r;
      if (qrow >= Lq) continue;
#pragma unroll
      for (int dt = 0; dt < NT; ++dt)
        if (DP == 64 || 16 * dt + lo < Dr)
          op[(int64_t)qrow * o_sl + 16 * dt + lo] = f2bf(acc_o[st][dt][r] * invl_r[r]);
    }
    if (hi == 0 && q0 + lo < Lq)
      lse[bh * Lq + q0 + lo] = m_run[st] + __logf(l_run[st]);
  }
}

// ---------------------------------------------------------------------------
// Small-L fast path (VERDICT r01 #4 — CLIP text L=77 causal was the worst
// kernel in the zoo): at L <= 80 the general kernel is OVERHEAD-bound —
// its 4-wave workgroups spend most of their time in barriers/staging for a
// few nearly-empty tiles. Here one WAVE owns one whole (b,h) attention:
//   * grid = ceil(B*H/4), 4 independent waves per workgroup, ZERO barriers
//     (each wave reads only its own LDS slice; its own ds writes are
//     ordered by the compiler's lgkmcnt / the tr-asm's lgkmcnt(0));
//   * K and V staged once per wave into BLOCK images (row-fragment reads
//     for QK^T, tr_b16 reads for PV);
//   * single-pass softmax (all <= 80 keys at once - no online rescale);
//   * causal masking skips whole 16-key tiles above the diagonal.
// D = 64 only (every model-zoo tower with L <= 80 has head_dim 64).
// ---------------------------------------------------------------------------

template <bool CAUSAL>
__global__ __launch_bounds__(320) void attn_fwd_small_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    bf16* __restrict__ o, float* __restrict__ lse, int Lq, int Lk, float scale, int H,
    int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
    int64_t v_sb, int64_t v_sh, int64_t v_sl, int64_t o_sb, int64_t o_sh, int64_t o_sl,
    int64_t BH) {
  constexpr int D = 64;
  constexpr int LP = 96;       // padded key count (block images need 32-multiples)
  constexpr int PPITCH = 88;   // P-tile pitch. The PV A-frag reads key columns
                               // up to 95 (s=2 covers keys 64..95); cols >= 88
                               // alias the NEXT row's written (finite) P values,
                               // which is benign: they multiply V image rows
                               // 88..95, zero-padded. 88 beats 96 twice: the
                               // P-tile write stride (44 words) is 2-way bank
                               // conflicted vs 8-way at 96, and the smaller
                               // footprint fits 6 WGs/CU instead of 5.
  constexpr int PSTRIDE = 16 * PPITCH + 8;  // +8 zeroed shorts: the last row's
                                            // col-95 over-read stays in zeroed
                                            // LDS even for the last wave
  // One 5-wave workgroup per (b, h): wave w owns q-strip w (<= 5 strips at
  // L <= 80), the V block image is staged ONCE and shared (one barrier).
  // K lives in REGISTERS per wave (5 kt x 2 s fragments = 40 VGPR/lane).
  // The previous wave-per-(b,h) version looped the 5 strips serially in
  // one wave and topped out at 2 waves/SIMD — latency-exposed (68.8 TF/s
  // at CLIP-text L=77); strip-per-wave runs 5x the waves at the same LDS
  // footprint per WG (12 KiB V image + 5 x 2.77 KiB P tiles = 25.8 KiB).
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int lo = lane & 15, hi = lane >> 4;
  short* vb = reinterpret_cast<short*>(smem);
  short* pt = vb + LP * D + wave * PSTRIDE;

  const int64_t bh = blockIdx.x;
  // zero the P tile once: the PV step reads key columns beyond Lk whose P
  // is never written (their V rows are zero-padded, but garbage LDS can
  // hold NaN bits and NaN * 0 = NaN — seen as an intermittent test failure)
#pragma unroll
  for (int i = 0; i < (PSTRIDE / 8 + WAVE - 1) / WAVE; ++i) {
    const int idx = i * WAVE + lane;
    if (idx < PSTRIDE / 8) *reinterpret_cast<bf16x8_t*>(pt + idx * 8) = bf16x8_t{};
  }
  const int64_t b = bh / H, h = bh % H;
  const bf16* qp = q + b * q_sb + h * q_sh;
  const bf16* kp = k + b * k_sb + h * k_sh;
  const bf16* vp = v + b * v_sb + h * v_sh;
  bf16* op = o + b * o_sb + h * o_sh;

  // ---- stage V into the workgroup's shared block image (zero-padded) -----
  {
    const int t = (int)threadIdx.x;
    for (int idx = t; idx < LP * D / 8; idx += 320) {  // 8-short chunk: (key, d-oct)
      const int key = idx >> 3;
      const int d8 = (idx & 7) * 8;
      bf16x8_t vv_{};
      if (key < Lk) vv_ = *reinterpret_cast<const bf16x8_t*>(vp + (int64_t)key * v_sl + d8);
      *reinterpret_cast<bf16x8_t*>(vb + boff<D>(key, d8)) = vv_;
    }
  }
  const int nq = (Lq + 15) / 16;
  const int nkt = (Lk + 15) / 16;
  const int qs = wave;
  __syncthreads();  // V image visible to all waves
  if (qs < nq) {
    const int q0 = qs * 16;
    // ---- K fragments straight from global into registers (causal strips
    // stop at their diagonal tile) -----------------------------------------
    const int ktmax0 = CAUSAL ? min(nkt, qs + 1) : nkt;
    bf16x8_t kfr[5][2];
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
      const int key = 16 * kt + lo;
#pragma unroll
      for (int s = 0; s < 2; ++s)
        kfr[kt][s] = (kt < ktmax0 && key < Lk)
                         ? *reinterpret_cast<const bf16x8_t*>(kp + (int64_t)key * k_sl + 32 * s + hi * 8)
                         : bf16x8_t{};
    }
    const int qrow = min(q0 + lo, Lq - 1);
    const bf16x8_t qb0 = *reinterpret_cast<const bf16x8_t*>(qp + (int64_t)qrow * q_sl + hi * 8);
    const bf16x8_t qb1 = *reinterpret_cast<const bf16x8_t*>(qp + (int64_t)qrow * q_sl + 32 + hi * 8);

    // ---- S^T = K . Q^T over <= 5 16-key tiles ----------------------------
    const int ktmax = ktmax0;
    f32x4_t sc[5] = {};
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
      if (kt >= ktmax) continue;
      sc[kt] = MFMA16(kfr[kt][0], qb0, sc[kt]);
      sc[kt] = MFMA16(kfr[kt][1], qb1, sc[kt]);
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- single-pass softmax (full row in registers + 2 shuffles) --------
    const int q_idx = q0 + lo;
    float sv[20];
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * kt + hi * 4 + r;
        float x = sc[kt][r] * scale;
        if (kt >= ktmax || key >= Lk || (CAUSAL && key > q_idx)) x = -INFINITY;
        sv[4 * kt + r] = x;
      }
    }
    float mt = sv[0];
#pragma unroll
    for (int i = 1; i < 20; ++i) mt = fmaxf(mt, sv[i]);
    mt = fmaxf(mt, __shfl_xor(mt, 16, WAVE));
    mt = fmaxf(mt, __shfl_xor(mt, 32, WAVE));
    float psum = 0.f;
#pragma unroll
    for (int i = 0; i < 20; ++i) {
      const float p = (sv[i] == -INFINITY) ? 0.f : __expf(sv[i] - mt);
      sv[i] = p;
      psum += p;
    }
    psum += __shfl_xor(psum, 16, WAVE);
    psum += __shfl_xor(psum, 32, WAVE);

    // ---- P (bf16) -> wave P-tile: [q = lo][key = 16kt + 4hi + r] ---------
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
      bf16x4 pk;
#pragma unroll
      for (int r = 0; r < 4; ++r) pk[r] = f2bfs(sv[4 * kt + r]);
      *reinterpret_cast<bf16x4*>(pt + lo * PPITCH + 16 * kt + hi * 4) = pk;
    }

    // ---- O = P . V (A = P rows, B = V^T via tr reads) --------------------
    f32x4_t acc_o[4] = {};
    const int kv_hi = CAUSAL ? min(Lk, q0 + 16) : Lk;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      if (32 * s >= kv_hi) continue;
      bf16x8_t vbf[4];
      const lds_cp bbase = (lds_cp)(const void*)(vb + s * 32 * D) + lane * 8;
      tr_frag_x4(bbase, vbf);
      const bf16x8_t pa = *reinterpret_cast<const bf16x8_t*>(pt + lo * PPITCH + 32 * s + hi * 8);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) acc_o[dt] = MFMA16(pa, vbf[dt], acc_o[dt]);
      __builtin_amdgcn_s_setprio(0);
    }

    // ---- epilogue ---------------------------------------------------------
    const float invl = psum > 0.f ? 1.f / psum : 0.f;
    float invl_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) invl_r[r] = __shfl(invl, hi * 4 + r, WAVE);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qr = q0 + hi * 4 + r;
      if (qr >= Lq) continue;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        op[(int64_t)qr * o_sl + 16 * dt + lo] = f2bf(acc_o[dt][r] * invl_r[r]);
    }
    if (hi == 0 && q0 + lo < Lq) lse[bh * Lq + q0 + lo] = mt + __logf(psum);
  }
}

}  // namespace

std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                    bool causal, double scale) {
  // q,k,v: (B,H,L,64) views whose innermost dim is contiguous, head stride
  // is 64 and L-row stride is uniform — covers both contiguous BHLD and the
  // un-copied (B,L,H,64) / fused-qkv (B,L,3,H,64) layouts.
  TORCH_CHECK(q.is_cuda());
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16, "attn_fwd: bf16 only, got ", q.scalar_type());
  TORCH_CHECK(q.dim() == 4, "attn_fwd: (B,H,L,D) expected");
  const int Dr = q.size(3);
  TORCH_CHECK(Dr == 64 || Dr == 72 || Dr == 80 || Dr == 96 || Dr == 128,
              "attn_fwd: head_dim must be one of {64,72,80,96,128}, got ", Dr);
  const int DP = Dr <= 64 ? 64 : (Dr <= 96 ? 96 : 128);
  const int B = q.size(0), H = q.size(1), Lq = q.size(2), Lk = k.size(2);
  TORCH_CHECK(k.size(0) == B && k.size(1) == H && v.size(2) == Lk);
  for (auto* t : {&q, &k, &v})
    TORCH_CHECK(t->stride(3) == 1, "attn_fwd: innermost dim must be contiguous");
  // O written in (B,L,H,64) memory order so the model's (B,L,H*64) reshape is
  // a free view (no permute copy)
  auto o_storage = torch::empty({B, Lq, H, Dr}, q.options());
  auto o = o_storage.permute({0, 2, 1, 3});
  auto lse = torch::empty({B, H, Lq}, q.options().dtype(torch::kFloat32));
  // 2 strips everywhere (3 waves/SIMD occupancy): the early-r02 measurement
  // that had 4 winning at L=197 no longer holds after the block-image /
  // double-buffer rework (L=197: 160 -> 171 TF/s at nstrip 2; L=257 with 4
  // is far worse, 207 -> 168). JIMM_AMD_ATTN_NSTRIP overrides for A/B.
  const int ntq = (Lq + QBLK - 1) / QBLK;
  int nstrip = 2;
  if (DP == 64) {
    if (const char* e = getenv("JIMM_AMD_ATTN_NSTRIP")) nstrip = (std::string(e) == "2") ? 2 : 4;
  }
  const dim3 grid((ntq + nstrip - 1) / nstrip, (unsigned)((int64_t)B * H));
  const size_t shmem =
      (2 * (KVBLK * DP + KVBLK * (DP + 8)) + 4 * 16 * (DP + 8)) * sizeof(short);
  auto stream = at::hip::getCurrentHIPStream();
#define ATTN_ARGS                                                                          \
                     reinterpret_cast<const bf16*>(q.data_ptr()),                          \
                     reinterpret_cast<const bf16*>(k.data_ptr()),                          \
                     reinterpret_cast<const bf16*>(v.data_ptr()),                          \
                     reinterpret_cast<bf16*>(o_storage.data_ptr()), lse.data_ptr<float>(), \
                     Lq, Lk, (float)scale, H, Dr, q.stride(0), q.stride(1), q.stride(2),   \
                     k.stride(0), k.stride(1), k.stride(2),                                \
                     v.stride(0), v.stride(1), v.stride(2),                                \
                     o.stride(0), o.stride(1), o.stride(2)
  // small-L fast path: one wave per (b,h), no barriers (L <= 80, D = 64)
  if (Dr == 64 && Lq == Lk && Lk <= 80) {
    const int64_t BH = (int64_t)B * H;
    const dim3 sgrid((unsigned)BH);  // one 5-wave WG per (b, h)
    const size_t sshmem = (96 * 64 + 5 * (16 * 88 + 8)) * sizeof(short);
#define SMALL_ARGS                                                                         \
                     reinterpret_cast<const bf16*>(q.data_ptr()),                          \
                     reinterpret_cast<const bf16*>(k.data_ptr()),                          \
                     reinterpret_cast<const bf16*>(v.data_ptr()),                          \
                     reinterpret_cast<bf16*>(o_storage.data_ptr()), lse.data_ptr<float>(), \
                     Lq, Lk, (float)scale, H, q.stride(0), q.stride(1), q.stride(2),       \
                     k.stride(0), k.stride(1), k.stride(2),                                \
                     v.stride(0), v.stride(1), v.stride(2),                                \
                     o.stride(0), o.stride(1), o.stride(2), BH
    if (causal)
      hipLaunchKernelGGL((attn_fwd_small_kernel<true>), sgrid, dim3(320), sshmem, stream,
                         SMALL_ARGS);
    else
      hipLaunchKernelGGL((attn_fwd_small_kernel<false>), sgrid, dim3(320), sshmem, stream,
                         SMALL_ARGS);
#undef SMALL_ARGS
    return {o, lse};
  }
#define ATTN_LAUNCH(C)                                                                     \
  do {                                                                                     \
    if (DP == 128)                                                                         \
      launch_lds<attn_fwd_kernel<C, 2, 128>>(grid, dim3(256), shmem, shmem, stream, ATTN_ARGS); \
    else if (DP == 96)                                                                     \
      launch_lds<attn_fwd_kernel<C, 2, 96>>(grid, dim3(256), shmem, shmem, stream, ATTN_ARGS);  \
    else if (nstrip == 2)                                                                  \
      launch_lds<attn_fwd_kernel<C, 2, 64>>(grid, dim3(256), shmem, shmem, stream, ATTN_ARGS);  \
    else                                                                                   \
      launch_lds<attn_fwd_kernel<C, 4, 64>>(grid, dim3(256), shmem, shmem, stream, ATTN_ARGS);  \
  } while (0)
  if (causal) ATTN_LAUNCH(true); else ATTN_LAUNCH(false);
#undef ATTN_LAUNCH
#undef ATTN_ARGS
  return {o, lse};
}
