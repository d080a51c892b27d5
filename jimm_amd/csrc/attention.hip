// K5 — flash-style attention forward for CDNA4 (gfx950), bf16, head_dim 64.
//
// Covers every attention in the model zoo: self-attention
// L in {50..1024} (ViT/CLIP/SigLIP towers, all with head_dim 64 since
// heads = width/64 — clip.py:60), causal masking for the CLIP text tower
// (clip.py:62), and the MAP head's Lq=1 cross-attention (K9).
//
// Design (one workgroup = 4 waves = NSTRIP strips of 64 q rows, 16 rows per
// wave and strip; grid = (ceil(ceil(Lq/64)/NSTRIP), B*H)):
//   * "swapped" QK^T: S^T = mfma(A=K_tile, B=Q^T) so each lane's softmax
//     row stats live in-lane + 2 shuffles (no serial-lane softmax — CDNA
//     guide common-mistake #6);
//   * K staged row-major in LDS, V staged as a block image whose transposed
//     reads (ds_read_b64_tr_b16) deliver the PV mfma's B-fragments;
//   * P routed through a per-wave LDS tile (padded rows, +8 shorts) to
//     re-shape from the S^T C-layout into the PV A-fragment layout;
//   * online softmax with running (m, l) per q row; lse = m + log(l)
//     saved for the backward (recompute) pass.
// Two single-launch kernels take over where a whole (b, h) fits one
// workgroup: attn_fwd_small_kernel (Lq == Lk <= 80) and
// attn_fwd_resident_kernel (81 <= Lq == Lk <= 256, non-causal, ViT-B L=197);
// both D = 64, see their header comments and the dispatch in attn_fwd.
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

constexpr int QBLK = 64;    // q rows per strip (16 per wave)
// q strips per workgroup: 2 keeps 3 waves/SIMD at every head dim and staging
// length (4 strips halve the K/V staging passes but drop to 2 waves/SIMD and
// measured slower everywhere: L=257 207 -> 168 TF/s)
constexpr int NSTRIP = 2;
constexpr int KVBLK = 64;   // keys per LDS tile

// Head dims beyond 64: the kernel is templated on the
// padded head dim DP and loads through ld8g<DP> (mfma.h).
//
// V block image (boff<DP>, mfma.h): [64 key][DP d], written with vector
// ds_write_b128 from the row-major staging registers and read as PV
// B-fragments with tr_frags at per-lane address base + lane*8 B.

template <bool CAUSAL, int DP>
__global__ __launch_bounds__(256) void attn_fwd_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    bf16* __restrict__ o, float* __restrict__ lse, int Lq, int Lk, float scale, int H, int Dr,
    hstride q_s, hstride k_s, hstride v_s, hstride o_s) {
  // Strides are those of the (B,H,L,D) views; the innermost dim is
  // contiguous. Covers contiguous BHLD, (B,L,H,D) and fused-qkv (B,L,3,H,D)
  // layouts with no permute copies.
  //
  // Each workgroup covers up to NSTRIP x 64 q rows of one (b,h): K/V tiles
  // are staged ONCE per kv tile for all strips (one strip per workgroup is
  // 4x redundant global traffic at L=197, ~125 of its 213 us
  // bandwidth-bound). T14 split staging; each wave keeps NSTRIP
  // online-softmax states.
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
  // cyclic strip -> q-tile mapping: strip t covers q tile
  // (blockIdx.x + t*gridDim.x) — balances ragged L (a blocked mapping gives
  // the last workgroup a nearly-empty supertile, e.g. 1 of 256 rows at L=257)
  const int ntq = (Lq + QBLK - 1) / QBLK;

  const bf16* qp = head_ptr(q, q_s, bh, H);
  const bf16* kp = head_ptr(k, k_s, bh, H);
  const bf16* vp = head_ptr(v, v_s, bh, H);
  bf16* op = head_ptr(o, o_s, bh, H);

  // ---- load Q fragments for every strip (B-operand of the swapped QK^T) --
  // strip t covers q rows [q_base + t*64, +64); this wave's rows:
  // q0(t) = q_base + t*64 + wave*16; B[d][q] = Q[q0+lo][32*s + hi*8 + j]
  bf16x8 qb[NSTRIP][NS];
  int nactive = 0;
#pragma unroll
  for (int t = 0; t < NSTRIP; ++t) {
    const int ti = blockIdx.x + t * gridDim.x;
    if (ti < ntq) nactive = t + 1;
    const int qrow = min(min(ti, ntq - 1) * QBLK + wave * 16 + lo, Lq - 1);
#pragma unroll
    for (int s = 0; s < NS; ++s)
      qb[t][s] = ld8g<DP>(qp + (int64_t)qrow * q_s.l, 32 * s + hi * 8, Dr);
  }

  short* my_p = p_lds + wave * 16 * LDS_PITCH;

  f32x4 acc_o[NSTRIP][NT] = {};  // O tiles: rows q = hi*4+r, cols d = 16*dt+lo
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
  bf16x8 kreg[NCG][2], vreg[NCG][2];
  bool st_valid;
  auto load_tile_regs = [&](int kv0) {
    const int key = kv0 + st_row;
    st_valid = key < Lk;
    const int krow = min(key, Lk - 1);
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
      const int c0 = cg * 64 + st_c0;
      if (c0 >= DP) continue;
      kreg[cg][0] = ld8g<DP>(kp + (int64_t)krow * k_s.l, c0, Dr);
      kreg[cg][1] = ld8g<DP>(kp + (int64_t)krow * k_s.l, c0 + 8, Dr);
      vreg[cg][0] = ld8g<DP>(vp + (int64_t)krow * v_s.l, c0, Dr);
      vreg[cg][1] = ld8g<DP>(vp + (int64_t)krow * v_s.l, c0 + 8, Dr);
    }
  };
  auto write_tile = [&](int buf) {
    const int bo = buf * IMGSF;
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
      const int c0 = cg * 64 + st_c0;
      if (c0 >= DP) continue;
      const bf16x8 k0 = st_valid ? kreg[cg][0] : bf16x8{};
      const bf16x8 k1 = st_valid ? kreg[cg][1] : bf16x8{};
      const bf16x8 v0 = st_valid ? vreg[cg][0] : bf16x8{};
      const bf16x8 v1 = st_valid ? vreg[cg][1] : bf16x8{};
      *reinterpret_cast<bf16x8*>(k_lds + bo + st_row * LDS_PITCH + c0) = k0;
      *reinterpret_cast<bf16x8*>(k_lds + bo + st_row * LDS_PITCH + c0 + 8) = k1;
      *reinterpret_cast<bf16x8*>(vt_lds + bo + boff<DP>(st_row, c0)) = v0;
      *reinterpret_cast<bf16x8*>(vt_lds + bo + boff<DP>(st_row, c0 + 8)) = v1;
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
      f32x4 sc[4] = {};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (kv0 + 16 * t >= kv_hi) continue;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const bf16x8 ka = row_frag(k_lds + sbo, 16 * t + lo, LDS_PITCH, s, hi);
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
        bf16x8 vb[NT];
        tr_frags<NT>((lds_cp)(const void*)(vt_lds + sbo + s * 32 * DP) + lane * 8, vb);
        const bf16x8 pa = row_frag(my_p, lo, LDS_PITCH, s, hi);
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
          op[(int64_t)qrow * o_s.l + 16 * dt + lo] = f2bf(acc_o[st][dt][r] * invl_r[r]);
    }
    if (hi == 0 && q0 + lo < Lq)
      lse[bh * Lq + q0 + lo] = m_run[st] + __logf(l_run[st]);
  }
}

// ---------------------------------------------------------------------------
// Small-L fast path (VERDICT r01 #4 — CLIP text L=77 causal was the worst
// kernel in the zoo): at L <= 80 the general kernel is OVERHEAD-bound —
// its 4-wave workgroups spend most of their time in barriers/staging for a
// few nearly-empty tiles. Here one 5-wave workgroup owns one whole (b,h):
//   * grid = B*H; wave w owns the 16-query strip w (<= 5 strips at L <= 80);
//   * V staged once into a shared BLOCK image (tr_b16 reads for PV), ONE
//     barrier; K lives in registers per wave (5 kt x 2 s fragments =
//     40 VGPR/lane), straight from global;
//   * single-pass softmax (all <= 80 keys at once - no online rescale);
//   * causal masking skips whole 16-key tiles above the diagonal.
// Strip-per-wave keeps 5x the waves of a wave-per-(b,h) layout in flight at
// the same LDS footprint per workgroup (12 KiB V image + 5 x 2.77 KiB P
// tiles = 25.8 KiB); the serial layout topped out at 2 waves/SIMD and was
// latency-exposed.
// D = 64 only (every model-zoo tower with L <= 80 has head_dim 64).
// ---------------------------------------------------------------------------

template <bool CAUSAL>
__global__ __launch_bounds__(320) void attn_fwd_small_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    bf16* __restrict__ o, float* __restrict__ lse, int Lq, int Lk, float scale, int H,
    hstride q_s, hstride k_s, hstride v_s, hstride o_s) {
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
    if (idx < PSTRIDE / 8) *reinterpret_cast<bf16x8*>(pt + idx * 8) = bf16x8{};
  }
  const bf16* qp = head_ptr(q, q_s, bh, H);
  const bf16* kp = head_ptr(k, k_s, bh, H);
  const bf16* vp = head_ptr(v, v_s, bh, H);
  bf16* op = head_ptr(o, o_s, bh, H);

  // ---- stage V into the workgroup's shared block image (zero-padded) -----
  {
    const int t = (int)threadIdx.x;
    for (int idx = t; idx < LP * D / 8; idx += 320) {  // 8-short chunk: (key, d-oct)
      const int key = idx >> 3;
      const int d8 = (idx & 7) * 8;
      bf16x8 vv_{};
      if (key < Lk) vv_ = *reinterpret_cast<const bf16x8*>(vp + (int64_t)key * v_s.l + d8);
      *reinterpret_cast<bf16x8*>(vb + boff<D>(key, d8)) = vv_;
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
    bf16x8 kfr[5][2];
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
      const int key = 16 * kt + lo;
#pragma unroll
      for (int s = 0; s < 2; ++s)
        kfr[kt][s] = (kt < ktmax0 && key < Lk)
                         ? *reinterpret_cast<const bf16x8*>(kp + (int64_t)key * k_s.l + 32 * s + hi * 8)
                         : bf16x8{};
    }
    const int qrow = min(q0 + lo, Lq - 1);
    const bf16x8 qb0 = *reinterpret_cast<const bf16x8*>(qp + (int64_t)qrow * q_s.l + hi * 8);
    const bf16x8 qb1 = *reinterpret_cast<const bf16x8*>(qp + (int64_t)qrow * q_s.l + 32 + hi * 8);

    // ---- S^T = K . Q^T over <= 5 16-key tiles ----------------------------
    const int ktmax = ktmax0;
    f32x4 sc[5] = {};
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
    f32x4 acc_o[4] = {};
    const int kv_hi = CAUSAL ? min(Lk, q0 + 16) : Lk;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      if (32 * s >= kv_hi) continue;
      bf16x8 vbf[4];
      const lds_cp bbase = (lds_cp)(const void*)(vb + s * 32 * D) + lane * 8;
      tr_frag_x4(bbase, vbf);
      const bf16x8 pa = row_frag(pt, lo, PPITCH, s, hi);
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
        op[(int64_t)qr * o_s.l + 16 * dt + lo] = f2bf(acc_o[dt][r] * invl_r[r]);
    }
    if (hi == 0 && q0 + lo < Lq) lse[bh * Lq + q0 + lo] = mt + __logf(psum);
  }
}

// ---------------------------------------------------------------------------
// Resident forward (Lq == Lk = L, 81 <= L <= 256, D = 64, non-causal; the
// domain of attn_bwd_resident_kernel, whose phase 1 this is without dP and
// delta). One workgroup per (b, h) with NBLK = ceil(L/32) waves; wave w owns
// the 16-query strips w and w + NBLK. K and V are staged ONCE into two
// natural-order block images (noff, mfma.h) with zero rows at and above L,
// and nothing else lives in LDS: 57 344 B at L = 197, 65 536 B at L = 256,
// so two workgroups share a CU and one loads or stores while the other
// computes. The tiled kernel at L = 197 runs two workgroups per head that
// both stage all of K and V, pads 197 rows to 256 and 197 keys to 256 with a
// barrier every 64, sends P through an LDS tile and rescales O per kv tile.
// Per strip:
//   S^T = K.Q^T with ds_read_b128 A-fragments of the K image and the strip's
//     Q rows in registers as B-fragments. ALL of the strip's scores stay in
//     registers (2*NBLK tiles, 64 VGPRs at NBLK = 8; NBLK is a template
//     argument so every index is a compile-time constant), so the softmax is
//     one max, one exp pass and no rescale. Query = lane lo: the statistics
//     are in-lane over (tile, r) plus __shfl_xor 16 and 32. (An online
//     softmax over a run-time block loop was built too and measured 10-28 %
//     slower at every L: profiles/attn_fwd_resident_NOTES.md.)
//   Only the last 32-key block can hold keys >= L; they are masked to -inf
//   by key index (a zero image row scores 0, not -inf). Padded query rows
//   take m = +inf, so their P is exact 0 too.
//   O^T += V^T.P^T: the tr_frag_x4 fragment of the V image is the A operand
//     and the bf16 P fragment built from two accumulator tiles the B operand
//     (see the backward kernel's header for the slot permutation), so the
//     accumulators hold transposed tiles: lane = query lo, d = 16dt + 4hi + r.
//     1/l is in-lane and the strip is stored as four 8-byte writes.
// exp runs as v_exp_f32 on scores pre-multiplied by scale*log2(e); lse is
// converted back to natural units.
// Every global load is clamped to row L-1 and every store guarded by
// row < L. The one barrier and every tr read are outside divergent control
// flow (the strip skip is wave-uniform), so EXEC is all ones at each
// ds_read_b64_tr_b16.
// ---------------------------------------------------------------------------

template <int NBLK>
__global__ __launch_bounds__(512, 4) void attn_fwd_resident_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    bf16* __restrict__ o, float* __restrict__ lse, int L, float scale, int H, hstride q_s,
    hstride k_s, hstride v_s, hstride o_s) {
  constexpr int D = 64;
  constexpr int LP = 32 * NBLK;  // image rows: whole 32-row blocks
  constexpr int IMG = LP * D;
  constexpr int NTHR = 64 * NBLK;  // the image has exactly 4 16-B chunks per thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* imgK = reinterpret_cast<short*>(smem);
  short* imgV = imgK + IMG;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int lo = lane & 15, hi = lane >> 4;
  const int64_t bh = blockIdx.x;
  const bf16* qp = head_ptr(q, q_s, bh, H);
  const bf16* kp = head_ptr(k, k_s, bh, H);
  const bf16* vp = head_ptr(v, v_s, bh, H);

  // ---- both strips' Q rows (B-fragments), in flight under the staging -------
  bf16x8 qb[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int srow = min(16 * (wave + i * NBLK) + lo, L - 1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
      qb[i][s] = *reinterpret_cast<const bf16x8*>(qp + (int64_t)srow * q_s.l + 32 * s + hi * 8);
  }

  // ---- stage K, V ------------------------------------------------------------
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = tid + it * NTHR;
    const int row = idx >> 3, d8 = (idx & 7) * 8;
    const int rc = min(row, L - 1);
    bf16x8 kk = *reinterpret_cast<const bf16x8*>(kp + (int64_t)rc * k_s.l + d8);
    bf16x8 vv = *reinterpret_cast<const bf16x8*>(vp + (int64_t)rc * v_s.l + d8);
    if (row >= L) kk = vv = bf16x8{};
    const int off = noff(row, d8);
    *reinterpret_cast<bf16x8*>(imgK + off) = kk;
    *reinterpret_cast<bf16x8*>(imgV + off) = vv;
  }
  __syncthreads();

  const float c = scale * 1.44269504088896340736f;  // scores in log2 units
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int s0 = 16 * (wave + i * NBLK);
    if (s0 >= L) continue;  // wave-uniform
    const bool sok = s0 + lo < L;

    // ---- S^T = K . Q^T, all 2*NBLK key tiles ---------------------------------
    f32x4 sc[NBLK][2];
#pragma unroll
    for (int kb = 0; kb < NBLK; ++kb) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        sc[kb][t] = f32x4{};
        // whole 16-key tile is padding (wave-uniform; masked below)
        if (kb == NBLK - 1 && 32 * kb + 16 * t >= L) continue;
        bf16x8 ka[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
          ka[s] = *reinterpret_cast<const bf16x8*>(
              imgK + noff(32 * kb + 16 * t + lo, 32 * s + hi * 8));
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < 2; ++s) sc[kb][t] = MFMA16(ka[s], qb[i][s], sc[kb][t]);
        __builtin_amdgcn_s_setprio(0);
      }
    }

    // ---- row max over every key (query = lane lo) ----------------------------
    float m = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < NBLK; ++kb) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = sc[kb][t][r] * c;
          if (kb == NBLK - 1 && 32 * kb + 16 * t + 4 * hi + r >= L) x = -INFINITY;
          sc[kb][t][r] = x;
          m = fmaxf(m, x);
        }
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, WAVE));
    m = fmaxf(m, __shfl_xor(m, 32, WAVE));
    const float msub = sok ? m : INFINITY;  // padded query rows: P = exp2(-inf) = 0

    // ---- P = exp2(S - m) 32 keys at a time; O^T += V^T . P^T -----------------
    float lsum = 0.f;
    f32x4 acc[4] = {};
#pragma unroll
    for (int kb = 0; kb < NBLK; ++kb) {
      bf16x8 pf;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(sc[kb][t][r] - msub);
          lsum += p;
          pf[4 * t + r] = f2bfs(p);
        }
      }
      bf16x8 vfr[4];
      tr_frag_x4((lds_cp)(const void*)(imgV + kb * 32 * D) + lane * 8, vfr);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) acc[dt] = MFMA16(vfr[dt], pf, acc[dt]);
      __builtin_amdgcn_s_setprio(0);
    }
    lsum += __shfl_xor(lsum, 16, WAVE);
    lsum += __shfl_xor(lsum, 32, WAVE);

    // acc holds O^T tiles: lane = query lo, d = 16dt + 4hi + r -> 8-byte stores
    if (sok) {
      const float invl = 1.f / lsum;
      bf16* op = head_ptr(o, o_s, bh, H) + (int64_t)(s0 + lo) * o_s.l + 4 * hi;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        bf16x4 pk;
#pragma unroll
        for (int r = 0; r < 4; ++r) pk[r] = f2bfs(acc[dt][r] * invl);
        *reinterpret_cast<bf16x4*>(op + 16 * dt) = pk;
      }
      if (hi == 0) lse[bh * L + s0 + lo] = m * 0.69314718055994530942f + __logf(lsum);
    }
  }
}

}  // namespace

std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                    bool causal, double scale, std::string path) {
  // q,k,v: (B,H,L,D) views whose innermost dim is contiguous — covers both
  // contiguous BHLD and the un-copied (B,L,H,D) / fused-qkv (B,L,3,H,D)
  // layouts.
  check_attn_args("attn_fwd", {{"q", q}}, {{"k", k}, {"v", v}});
  const int Dr = q.size(3);
  const int DP = Dr <= 64 ? 64 : (Dr <= 96 ? 96 : 128);
  const int B = q.size(0), H = q.size(1), Lq = q.size(2), Lk = k.size(2);
  // path: "auto" picks small (L <= 80) / resident (81..RES_LMAX) / tiled;
  // "tiled" is auto without the resident kernel; "resident" fails outside
  // its domain
  TORCH_CHECK(path == "auto" || path == "tiled" || path == "resident",
              "attn_fwd: path must be auto, tiled or resident, got ", path);
  const bool aligned = res_aligned({&q, &k, &v});  // o is allocated below, aligned
  const bool resident_ok = Dr == 64 && Lq == Lk && !causal && Lk >= RES_LMIN &&
                           Lk <= RES_LMAX && aligned;
  TORCH_CHECK(path != "resident" || resident_ok,
              "attn_fwd: path=resident needs D == 64, Lq == Lk, non-causal, ", RES_LMIN,
              " <= L <= ", RES_LMAX, " and 16-byte aligned rows; got D=", Dr, " Lq=", Lq,
              " Lk=", Lk, " causal=", causal, " aligned=", aligned);
  // O written in (B,L,H,D) memory order so the model's (B,L,H*D) reshape is
  // a free view (no permute copy)
  auto o = torch::empty({B, Lq, H, Dr}, q.options()).permute({0, 2, 1, 3});
  auto lse = torch::empty({B, H, Lq}, q.options().dtype(torch::kFloat32));
  const unsigned BH = (unsigned)((int64_t)B * H);
  auto stream = at::hip::getCurrentHIPStream();
  if (path != "tiled" && resident_ok) {
    // one wave per 32 rows (two 16-row strips each); K and V images only.
    // The LDS limit is raised once, to the largest supported L.
    const int nblk = (Lk + 31) / 32;
    const size_t rshmem = (size_t)2 * nblk * 32 * 64 * sizeof(short);
    constexpr size_t rshmem_max = (size_t)2 * RES_LMAX * 64 * sizeof(short);
    with_int<3, 4, 5, 6, 7, 8>(nblk, "resident block count", [&](auto nb) {
      launch_lds<attn_fwd_resident_kernel<decltype(nb)::value>>(
          dim3(BH), dim3(nblk * WAVE), rshmem, rshmem_max, stream, bf16_ptr(q), bf16_ptr(k),
          bf16_ptr(v), bf16_ptr(o), lse.data_ptr<float>(), Lk, (float)scale, H, hstrides(q),
          hstrides(k), hstrides(v), hstrides(o));
    });
    return {o, lse};
  }
  with_flags(
      [&](auto c) {
        constexpr bool C = decltype(c)::value;
        // small-L fast path: one 5-wave workgroup per (b,h) (L <= 80, D = 64)
        if (Dr == 64 && Lq == Lk && Lk <= 80) {
          const size_t shmem = (96 * 64 + 5 * (16 * 88 + 8)) * sizeof(short);
          launch_lds<attn_fwd_small_kernel<C>>(
              dim3(BH), dim3(320), shmem, shmem, stream, bf16_ptr(q), bf16_ptr(k), bf16_ptr(v),
              bf16_ptr(o), lse.data_ptr<float>(), Lq, Lk, (float)scale, H, hstrides(q),
              hstrides(k), hstrides(v), hstrides(o));
          return;
        }
        const int ntq = (Lq + QBLK - 1) / QBLK;
        const size_t shmem =
            (2 * (KVBLK * DP + KVBLK * (DP + 8)) + 4 * 16 * (DP + 8)) * sizeof(short);
        with_int<64, 96, 128>(DP, "padded head dim", [&](auto dp) {
          launch_lds<attn_fwd_kernel<C, decltype(dp)::value>>(
              dim3((ntq + NSTRIP - 1) / NSTRIP, BH), dim3(256), shmem, shmem, stream,
              bf16_ptr(q), bf16_ptr(k), bf16_ptr(v), bf16_ptr(o), lse.data_ptr<float>(), Lq, Lk,
              (float)scale, H, Dr, hstrides(q), hstrides(k), hstrides(v), hstrides(o));
        });
      },
      causal);
  return {o, lse};
}
