// K15 — fused flash-attention backward for CDNA4 (gfx950), bf16, head_dim 64.
//
// Replaces the recompute-P composite (attention_bwd.hip + 5 rocBLAS batched
// GEMMs + .contiguous() copies) that the round-1 profile measured at
// ~15 ms/step for ViT-B/16 train (profiles/r01_NOTES.md). Two kernels, both
// recomputing P = exp(scale*S - lse) from the saved forward LSE:
//
//   attn_bwd_dkv_kernel — grid over (kv_tile, B*H): each workgroup owns 64
//     keys, loops over q tiles, accumulates dK/dV in MFMA registers, writes
//     them STRIDED straight into the fused dqkv buffer (no assembly copies).
//   attn_bwd_dq_kernel  — grid over (q_tile, B*H): each workgroup owns 64
//     q rows, loops over kv tiles, accumulates dQ. No atomics anywhere.
//
//   attn_d2_kernel      — D[b,h,l] = rowsum(dO * O), stride-aware fp32
//     (consumed by both kernels for dS = P*(dP - D)*scale).
//
// Two single-launch kernels take over where a whole (b, h) fits in LDS:
//   attn_bwd_small_kernel    — Lq == Lk <= 80
//   attn_bwd_resident_kernel — 81 <= Lq == Lk <= 256, non-causal (ViT-B L=197)
// (both D = 64; see their header comments and the dispatch in attn_bwd_fused).
//
// All tensor arguments are (B,H,L,64) *views* with arbitrary (b,h,l) strides
// and a contiguous innermost dim — q/k/v slices of the fused (B,L,3,H,64)
// QKV projection and (B,L,H,64)-storage dO/O are consumed with zero permute
// copies (the round-1 profile showed 3.9 ms/step of pure copy kernels).
//
// MFMA fragment conventions identical to attention.hip (verified on hardware
// by csrc/probe.hip + tests/test_kernels_gpu.py::test_mfma_probe):
//   A[i][k]: lane l holds A[l&15][(l>>4)*8 + j], j=0..7
//   B[k][j]: lane l holds B[(l>>4)*8 + j][l&15]
//   C[i][j]: lane l holds rows (l>>4)*4+r (r=0..3), col l&15

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "mfma.h"

namespace {

constexpr int BLK = 64;            // q rows / keys per workgroup tile

// Head dims beyond 64: padded-D template DP in {64,96,128}, ragged chunks
// guarded by ld8g<DP> (mfma.h). A tiled workgroup owns 2 tiles at DP=64,
// with the staged tile's fragments cached across them; DP>64 owns 1 tile and
// reads the fragments inline to stay inside the register budget.
constexpr int tiles_per_wg(int DP) { return DP == 64 ? 2 : 1; }

// Transposed operands come from block-format images: boff<ND> places an
// element, tr_frags / tr_frag_x4 read the fragments back (mfma.h).

// ---------------------------------------------------------------------------
// D = rowsum(dO * O), stride-aware
// ---------------------------------------------------------------------------

__global__ void attn_d2_kernel(const bf16* __restrict__ dO, const bf16* __restrict__ O,
                               float* __restrict__ Dv, int H, int L, int Dr, int64_t nrows,
                               hstride do_s, hstride o_s) {
  // 8 rows per wave (all 64 lanes loading): lane -> (sub-row l>>3, 8 cols)
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int wpb = blockDim.x / WAVE;
  const int sub = lane >> 3;          // 0..7 row within the wave's group
  const int c0 = (lane & 7) * 8;      // 8 elements per lane per 64-chunk
  for (int64_t base = ((int64_t)blockIdx.x * wpb + wave) * 8; base < nrows;
       base += (int64_t)gridDim.x * wpb * 8) {
    const int64_t row = base + sub;
    const int64_t rc = row < nrows ? row : nrows - 1;
    const int64_t b = rc / ((int64_t)H * L);
    const int h = (int)((rc / L) % H);
    const int l = (int)(rc % L);
    const bf16* a = dO + b * do_s.b + h * do_s.h + (int64_t)l * do_s.l;
    const bf16* o = O + b * o_s.b + h * o_s.h + (int64_t)l * o_s.l;
    float acc = 0.f;
    for (int cg = 0; cg < Dr; cg += 64) {
      if (cg + c0 + 8 > Dr) continue;
      float av[8], ov[8];
      vload_f32<8>(a + cg + c0, av);
      vload_f32<8>(o + cg + c0, ov);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += av[j] * ov[j];
    }
    // reduce across the 8 lanes of this sub-row
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) acc += __shfl_xor(acc, off, WAVE);
    if ((lane & 7) == 0 && row < nrows) Dv[row] = acc;
  }
}

// ---------------------------------------------------------------------------
// dK/dV kernel: workgroup owns keys [kv0, kv0+64); loops q tiles
// ---------------------------------------------------------------------------

template <bool CAUSAL, int DP>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ dO, const float* __restrict__ lse, const float* __restrict__ Dv,
    bf16* __restrict__ dk, bf16* __restrict__ dv, int Lq, int Lk, float scale, int H,
    int Dr, hstride q_s, hstride k_s, hstride v_s, hstride do_s, hstride dk_s, hstride dv_s) {
  // Each workgroup owns up to NKV kv tiles (cyclic tile mapping, like the
  // forward kernel) so the Q/dO images are staged ONCE for all of them (one
  // kv tile per workgroup is 4x redundant staging at L=197).
  // K/V live as per-strip A-FRAGMENTS in registers — no K/V LDS at all.
  // LDS: Q^T/dO^T (transposed) + Q/dO (row) images of the current q tile,
  // per-wave P/dS tile. ~46 KiB.
  constexpr int NKV = tiles_per_wg(DP);
  constexpr int PITCH = DP + 8;
  constexpr int NS = DP / 32;
  constexpr int NT = DP / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // staging images are DOUBLE-buffered: the write pass for tile it+1 runs
  // before/under tile it's MFMAs into the other buffer, so each q-tile
  // needs ONE __syncthreads instead of two (the single-buffer version
  // parked 41-44% of wave time at its write-drain barriers)
  constexpr int IMGS = 2 * BLK * DP + 2 * BLK * PITCH;  // per buffer
  short* qb_lds = reinterpret_cast<short*>(smem);   // Q  block image [64 q][DP d]
  short* dob_lds = qb_lds + BLK * DP;               // dO block image
  short* qr_lds = dob_lds + BLK * DP;               // Q    [64 q][PITCH] row image
  short* dor_lds = qr_lds + BLK * PITCH;            // dO   [64 q][PITCH]
  short* p_lds = reinterpret_cast<short*>(smem) + 2 * IMGS;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int lo = lane & 15, hi = lane >> 4;
  const int64_t bh = blockIdx.y;
  const int ntk = (Lk + BLK - 1) / BLK;

  const bf16* qp = head_ptr(q, q_s, bh, H);
  const bf16* kp = head_ptr(k, k_s, bh, H);
  const bf16* vp = head_ptr(v, v_s, bh, H);
  const bf16* dop = head_ptr(dO, do_s, bh, H);
  const float* lsep = lse + bh * Lq;
  const float* dvp_row = Dv + bh * Lq;

  // ---- per-strip K/V A-fragments straight from global (no LDS) ------------
  // strip s covers kv tile ti(s) = blockIdx.x + s*gridDim.x; this wave's 16
  // keys of that tile: rows 16*wave + lo. Invalid rows clamp; their P/dS
  // contributions are masked to zero and their stores are guarded.
  bf16x8 ka[NKV][NS], va[NKV][NS];
  int kvbase[NKV];
  int nactive = 0;
#pragma unroll
  for (int s = 0; s < NKV; ++s) {
    const int ti = blockIdx.x + s * gridDim.x;
    kvbase[s] = ti * BLK;
    if (ti < ntk) nactive = s + 1;
    const int key = min(min(ti, ntk - 1) * BLK + 16 * wave + lo, Lk - 1);
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      ka[s][t] = ld8g<DP>(kp + (int64_t)key * k_s.l, 32 * t + hi * 8, Dr);
      va[s][t] = ld8g<DP>(vp + (int64_t)key * v_s.l, 32 * t + hi * 8, Dr);
    }
  }

  short* my_p = p_lds + wave * 16 * PITCH;

  f32x4 acc_dk[NKV][NT] = {};  // rows key = 16*wave + hi*4+r, cols d = 16*dt+lo
  f32x4 acc_dv[NKV][NT] = {};

  // causal: the earliest kv tile of this WG bounds the first useful q tile
  const int q_start = CAUSAL ? (kvbase[0] / BLK) * BLK : 0;
  const int ntiles = (Lq - q_start + BLK - 1) / BLK;

  // per-thread staging slot for the Q/dO images
  constexpr int NCG = (DP + 63) / 64;
  const int st_row = tid / 4;
  const int st_c0 = (tid % 4) * 16;
  bf16x8 qreg[NCG][2], doreg[NCG][2];
  bool st_valid;
  auto load_stage_regs = [&](int q0) {
    const int qi = q0 + st_row;
    st_valid = qi < Lq;
    const int qr = min(qi, Lq - 1);
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
      if (cg * 64 + st_c0 >= DP) continue;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        qreg[cg][hh] = ld8g<DP>(qp + (int64_t)qr * q_s.l, cg * 64 + st_c0 + hh * 8, Dr);
        doreg[cg][hh] = ld8g<DP>(dop + (int64_t)qr * do_s.l, cg * 64 + st_c0 + hh * 8, Dr);
      }
    }
  };
  auto write_stage = [&](int buf) {
    const int bo = buf * IMGS;
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
      const int c0 = cg * 64 + st_c0;
      if (c0 >= DP) continue;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const bf16x8 qv = st_valid ? qreg[cg][hh] : bf16x8{};
        const bf16x8 dv2 = st_valid ? doreg[cg][hh] : bf16x8{};
        *reinterpret_cast<bf16x8*>(qr_lds + bo + st_row * PITCH + c0 + hh * 8) = qv;
        *reinterpret_cast<bf16x8*>(dor_lds + bo + st_row * PITCH + c0 + hh * 8) = dv2;
        *reinterpret_cast<bf16x8*>(qb_lds + bo + boff<DP>(st_row, c0 + hh * 8)) = qv;
        *reinterpret_cast<bf16x8*>(dob_lds + bo + boff<DP>(st_row, c0 + hh * 8)) = dv2;
      }
    }
  };

  load_stage_regs(q_start);
  write_stage(0);
  if (ntiles > 1) load_stage_regs(q_start + BLK);
  __syncthreads();

  for (int it = 0; it < ntiles; ++it) {
    const int q0 = q_start + it * BLK;
    const int sbo = (it & 1) * IMGS;  // this tile's staging buffer offset
    if (it + 1 < ntiles) {
      write_stage((it + 1) & 1);
      if (it + 2 < ntiles) load_stage_regs(q_start + (it + 2) * BLK);
    }
    // ---- B-fragments of Q^T and dO^T from the LDS row images (shared by
    // every kv strip) ------------------------------------------------------
    // DP==64 caches the q-tile fragments across the NKV strips; larger DP
    // reads them inline per use (the 4xNS cache would spill at NS=4)
    bf16x8 qb[DP == 64 ? 4 : 1][NS], dob[DP == 64 ? 4 : 1][NS];
    if constexpr (DP == 64) {
#pragma unroll
      for (int qt = 0; qt < 4; ++qt) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          qb[qt][s] = row_frag(qr_lds + sbo, 16 * qt + lo, PITCH, s, hi);
          dob[qt][s] = row_frag(dor_lds + sbo, 16 * qt + lo, PITCH, s, hi);
        }
      }
    }

#pragma unroll
    for (int sidx = 0; sidx < NKV; ++sidx) {
      if (sidx >= nactive) continue;
      const int kv0 = kvbase[sidx];
      if (CAUSAL && q0 + BLK - 1 < kv0) continue;  // whole tile above diagonal

      // ---- S^T = K . Q^T ; P^T = exp(scale*S^T - lse[q]) -----------------
      // this wave's keys start at key_min; q sub-tiles fully above the
      // causal diagonal (or beyond Lq) contribute P = dS = 0 — write zeros
      // and skip their MFMAs (at L=77 causal most sub-tiles are waste)
      const int key_min = kv0 + 16 * wave;
      // whole 16-key strip is padding (ragged last tile, e.g. keys 192..255
      // at L=197): every P/dS is zero and the dK/dV stores are key-guarded —
      // skip the strip's S/P/dS and MFMA work outright
      if (key_min >= Lk) continue;
      bf16x4 ds_stash[4];
#pragma unroll
      for (int qt = 0; qt < 4; ++qt) {
        const bool skip_qt =
            (CAUSAL && q0 + 16 * qt + 15 < key_min) || (q0 + 16 * qt >= Lq);
        if (skip_qt) {
          const bf16x4 z = {};
#pragma unroll
          for (int r = 0; r < 4; ++r) my_p[(hi * 4 + r) * PITCH + 16 * qt + lo] = 0;
          ds_stash[qt] = z;
          continue;
        }
        __builtin_amdgcn_s_setprio(1);
        f32x4 sc = {};
        f32x4 dpc = {};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          bf16x8 qf, dof;
          if constexpr (DP == 64) {
            qf = qb[qt][s];
            dof = dob[qt][s];
          } else {
            qf = row_frag(qr_lds + sbo, 16 * qt + lo, PITCH, s, hi);
            dof = row_frag(dor_lds + sbo, 16 * qt + lo, PITCH, s, hi);
          }
          sc = MFMA16(ka[sidx][s], qf, sc);
          dpc = MFMA16(va[sidx][s], dof, dpc);
        }
        __builtin_amdgcn_s_setprio(0);
        const int qi = q0 + 16 * qt + lo;
        const float l = lsep[min(qi, Lq - 1)];
        const float dcoef = dvp_row[min(qi, Lq - 1)];
        bf16x4 pk, dsk;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kv0 + 16 * wave + hi * 4 + r;
          float p = __expf(sc[r] * scale - l);
          if (qi >= Lq || key >= Lk || (CAUSAL && key > qi)) p = 0.f;
          pk[r] = f2bfs(p);
          dsk[r] = f2bfs(p * (dpc[r] - dcoef) * scale);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) my_p[(hi * 4 + r) * PITCH + 16 * qt + lo] = pk[r];
        ds_stash[qt] = dsk;
      }

      // ---- dV += P^T . dO  (A = P^T via LDS, B = dO^T via tr reads) ------
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if ((CAUSAL && q0 + 32 * s + 31 < key_min) || q0 + 32 * s >= Lq) continue;
        bf16x8 bfr[NT];
        tr_frags<NT>((lds_cp)(const void*)(dob_lds + sbo + s * 32 * DP) + lane * 8, bfr);
        const bf16x8 pa = row_frag(my_p, lo, PITCH, s, hi);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int dt = 0; dt < NT; ++dt) acc_dv[sidx][dt] = MFMA16(pa, bfr[dt], acc_dv[sidx][dt]);
        __builtin_amdgcn_s_setprio(0);
      }

      // ---- overwrite the wave tile with dS^T, then dK += dS^T . Q --------
#pragma unroll
      for (int qt = 0; qt < 4; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) my_p[(hi * 4 + r) * PITCH + 16 * qt + lo] = ds_stash[qt][r];
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if ((CAUSAL && q0 + 32 * s + 31 < key_min) || q0 + 32 * s >= Lq) continue;
        bf16x8 bfr[NT];
        tr_frags<NT>((lds_cp)(const void*)(qb_lds + sbo + s * 32 * DP) + lane * 8, bfr);
        const bf16x8 dsa = row_frag(my_p, lo, PITCH, s, hi);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int dt = 0; dt < NT; ++dt) acc_dk[sidx][dt] = MFMA16(dsa, bfr[dt], acc_dk[sidx][dt]);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    // double-buffered: tile it+1's write pass ran into the other buffer
    // before the MFMAs above; ONE barrier publishes it and retires this
    // tile's reads
    __syncthreads();
  }

  // ---- store dK, dV (strided, bf16) ---------------------------------------
  bf16* dkp = head_ptr(dk, dk_s, bh, H);
  bf16* dvp = head_ptr(dv, dv_s, bh, H);
#pragma unroll
  for (int sidx = 0; sidx < NKV; ++sidx) {
    if (sidx >= nactive) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = kvbase[sidx] + 16 * wave + hi * 4 + r;
      if (key >= Lk) continue;
#pragma unroll
      for (int dt = 0; dt < NT; ++dt) {
        if (DP != 64 && 16 * dt + lo >= Dr) continue;
        dkp[(int64_t)key * dk_s.l + 16 * dt + lo] = f2bf(acc_dk[sidx][dt][r]);
        dvp[(int64_t)key * dv_s.l + 16 * dt + lo] = f2bf(acc_dv[sidx][dt][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// dQ kernel: workgroup owns q rows [q0, q0+64); loops kv tiles
// ---------------------------------------------------------------------------

template <bool CAUSAL, int DP>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ dO, const float* __restrict__ lse, const float* __restrict__ Dv,
    bf16* __restrict__ dq, int Lq, int Lk, float scale, int H, int Dr, hstride q_s,
    hstride k_s, hstride v_s, hstride do_s, hstride dq_s) {
  // Each workgroup owns up to NQS q tiles (cyclic mapping) so the K images
  // are staged ONCE for all of them; Q/dO A-fragments live in registers per
  // strip. LDS: K^T + K/V row images of the current kv tile, per-wave dS
  // tile.
  constexpr int NQS = tiles_per_wg(DP);
  constexpr int PITCH = DP + 8;
  constexpr int NS = DP / 32;
  constexpr int NT = DP / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // double-buffered staging (as in the dkv kernel): one barrier per tile
  constexpr int IMGSQ = BLK * DP + 2 * BLK * PITCH;  // per buffer
  short* kb_lds = reinterpret_cast<short*>(smem);     // K block image [64 key][DP d]
  short* kr_lds = kb_lds + BLK * DP;                  // K   [64 key][PITCH]
  short* vr_lds = kr_lds + BLK * PITCH;               // V   [64 key][PITCH]
  short* ds_lds = reinterpret_cast<short*>(smem) + 2 * IMGSQ;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int lo = lane & 15, hi = lane >> 4;
  const int64_t bh = blockIdx.y;
  const int ntq = (Lq + BLK - 1) / BLK;

  const bf16* qp = head_ptr(q, q_s, bh, H);
  const bf16* kp = head_ptr(k, k_s, bh, H);
  const bf16* vp = head_ptr(v, v_s, bh, H);
  const bf16* dop = head_ptr(dO, do_s, bh, H);
  const float* lsep = lse + bh * Lq;
  const float* dvp_row = Dv + bh * Lq;

  // ---- per-strip Q/dO A-fragments + per-row lse/D -------------------------
  // strip s covers q tile ti(s) = blockIdx.x + s*gridDim.x; this wave's 16
  // q rows of that tile: rows 16*wave + ...
  bf16x8 qa[NQS][NS], doa[NQS][NS];
  float lse_r[NQS][4], d_r[NQS][4];
  int qbase[NQS];
  int nactive = 0;
#pragma unroll
  for (int s = 0; s < NQS; ++s) {
    const int ti = blockIdx.x + s * gridDim.x;
    qbase[s] = ti * BLK;
    if (ti < ntq) nactive = s + 1;
    const int q0 = min(ti, ntq - 1) * BLK + wave * 16;
    const int qrow = min(q0 + lo, Lq - 1);
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      qa[s][t] = ld8g<DP>(qp + (int64_t)qrow * q_s.l, 32 * t + hi * 8, Dr);
      doa[s][t] = ld8g<DP>(dop + (int64_t)qrow * do_s.l, 32 * t + hi * 8, Dr);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qi = min(q0 + hi * 4 + r, Lq - 1);
      lse_r[s][r] = lsep[qi];
      d_r[s][r] = dvp_row[qi];
    }
  }

  short* my_ds = ds_lds + wave * 16 * PITCH;
  f32x4 acc_dq[NQS][NT] = {};  // rows q = hi*4+r, cols d = 16*dt + lo

  // causal: only kv tiles up to the LAST active strip's diagonal are needed
  const int ti_max = blockIdx.x + (nactive - 1) * gridDim.x;
  const int kv_end = CAUSAL ? min(Lk, (ti_max + 1) * BLK) : Lk;
  const int ntiles = (kv_end + BLK - 1) / BLK;

  constexpr int NCG = (DP + 63) / 64;
  const int st_row = tid / 4;
  const int st_c0 = (tid % 4) * 16;
  bf16x8 kreg[NCG][2], vreg[NCG][2];
  bool st_valid;
  auto load_stage_regs = [&](int kv0) {
    const int key = kv0 + st_row;
    st_valid = key < Lk;
    const int kr = min(key, Lk - 1);
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
      if (cg * 64 + st_c0 >= DP) continue;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        kreg[cg][hh] = ld8g<DP>(kp + (int64_t)kr * k_s.l, cg * 64 + st_c0 + hh * 8, Dr);
        vreg[cg][hh] = ld8g<DP>(vp + (int64_t)kr * v_s.l, cg * 64 + st_c0 + hh * 8, Dr);
      }
    }
  };
  auto write_stage = [&](int buf) {
    const int bo = buf * IMGSQ;
#pragma unroll
    for (int cg = 0; cg < NCG; ++cg) {
      const int c0 = cg * 64 + st_c0;
      if (c0 >= DP) continue;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const bf16x8 kv2 = st_valid ? kreg[cg][hh] : bf16x8{};
        const bf16x8 vv2 = st_valid ? vreg[cg][hh] : bf16x8{};
        *reinterpret_cast<bf16x8*>(kr_lds + bo + st_row * PITCH + c0 + hh * 8) = kv2;
        *reinterpret_cast<bf16x8*>(vr_lds + bo + st_row * PITCH + c0 + hh * 8) = vv2;
        *reinterpret_cast<bf16x8*>(kb_lds + bo + boff<DP>(st_row, c0 + hh * 8)) = kv2;
      }
    }
  };

  load_stage_regs(0);
  write_stage(0);
  if (ntiles > 1) load_stage_regs(BLK);
  __syncthreads();

  for (int it = 0; it < ntiles; ++it) {
    const int kv0 = it * BLK;
    const int sbo = (it & 1) * IMGSQ;
    if (it + 1 < ntiles) {
      write_stage((it + 1) & 1);
      if (it + 2 < ntiles) load_stage_regs(kv0 + 2 * BLK);
    }
    // ---- B-fragments of K^T and V^T from the LDS row images (shared) -----
    bf16x8 kb[DP == 64 ? 4 : 1][NS], vb[DP == 64 ? 4 : 1][NS];
    if constexpr (DP == 64) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          kb[kt][s] = row_frag(kr_lds + sbo, 16 * kt + lo, PITCH, s, hi);
          vb[kt][s] = row_frag(vr_lds + sbo, 16 * kt + lo, PITCH, s, hi);
        }
      }
    }

#pragma unroll
    for (int sidx = 0; sidx < NQS; ++sidx) {
      if (sidx >= nactive) continue;
      const int q0s = qbase[sidx] + wave * 16;
      if (CAUSAL && kv0 >= qbase[sidx] + BLK) continue;  // tile above diagonal
      if (q0s >= Lq) continue;  // whole 16-query strip is padding

      // ---- S, P, dP, dS per 16-key tile ----------------------------------
      // key sub-tiles above this strip's causal diagonal or beyond Lk give
      // dS = 0: write zeros, skip the MFMAs
      const int q_max = q0s + 15;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const bool skip_kt =
            (CAUSAL && kv0 + 16 * kt > q_max) || (kv0 + 16 * kt >= Lk);
        if (skip_kt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) my_ds[(hi * 4 + r) * PITCH + 16 * kt + lo] = 0;
          continue;
        }
        __builtin_amdgcn_s_setprio(1);
        f32x4 sc = {};
        f32x4 dpc = {};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          bf16x8 kf, vf;
          if constexpr (DP == 64) {
            kf = kb[kt][s];
            vf = vb[kt][s];
          } else {
            kf = row_frag(kr_lds + sbo, 16 * kt + lo, PITCH, s, hi);
            vf = row_frag(vr_lds + sbo, 16 * kt + lo, PITCH, s, hi);
          }
          sc = MFMA16(qa[sidx][s], kf, sc);
          dpc = MFMA16(doa[sidx][s], vf, dpc);
        }
        __builtin_amdgcn_s_setprio(0);
        const int key = kv0 + 16 * kt + lo;
        bf16x4 dsk;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qi = q0s + hi * 4 + r;
          float p = __expf(sc[r] * scale - lse_r[sidx][r]);
          if (key >= Lk || (CAUSAL && key > qi)) p = 0.f;
          dsk[r] = f2bfs(p * (dpc[r] - d_r[sidx][r]) * scale);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) my_ds[(hi * 4 + r) * PITCH + 16 * kt + lo] = dsk[r];
      }

      // ---- dQ += dS . K (A = dS via LDS, B = K^T via tr reads) -----------
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if ((CAUSAL && kv0 + 32 * s > q_max) || kv0 + 32 * s >= Lk) continue;
        bf16x8 bfr[NT];
        tr_frags<NT>((lds_cp)(const void*)(kb_lds + sbo + s * 32 * DP) + lane * 8, bfr);
        const bf16x8 dsa = row_frag(my_ds, lo, PITCH, s, hi);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int dt = 0; dt < NT; ++dt) acc_dq[sidx][dt] = MFMA16(dsa, bfr[dt], acc_dq[sidx][dt]);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    // double-buffered: ONE barrier publishes tile it+1 and retires it
    __syncthreads();
  }

  // ---- store dQ (strided, bf16) -------------------------------------------
  bf16* dqp = head_ptr(dq, dq_s, bh, H);
#pragma unroll
  for (int sidx = 0; sidx < NQS; ++sidx) {
    if (sidx >= nactive) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qi = qbase[sidx] + wave * 16 + hi * 4 + r;
      if (qi >= Lq) continue;
#pragma unroll
      for (int dt = 0; dt < NT; ++dt)
        if (DP == 64 || 16 * dt + lo < Dr)
          dqp[(int64_t)qi * dq_s.l + 16 * dt + lo] = f2bf(acc_dq[sidx][dt][r]);
    }
  }
}


// ---------------------------------------------------------------------------
// Small-L fused backward (Lq == Lk <= 80, D = 64): ONE kernel replaces the
// d2 + dkv + dq trio, whose 64-wide tiles waste 1.7x padding at L = 77
// (CLIP text). One 5-wave workgroup per (b, h):
//   phase 1 (wave = 16-query strip): S^T = K.Q^T and dP^T = V.dO^T with K/V
//     in REGISTERS (40 VGPR each) and Q/dO rows read direct from global;
//     P = exp(scale*S - lse) (no max pass -- lse saved by the forward);
//     delta = rowsum(P o dP) (== rowsum(dO o O), so no O re-read);
//     dS = P o (dP - delta) * scale; the strip's dQ = dS @ K via tr-read
//     B-fragments of a shared K block image.
//   phase 2 (wave = 16-key strip): dK = dS^T @ Q and dV = P^T @ dO from
//     row-major P^T / dS^T LDS tiles (written in-register-order by phase 1)
//     against tr-read fragments of shared Q / dO block images (the K image
//     slot is restaged with dO between phases).
// Tile pitch 88 < 96: over-reads past col 87 alias the next row's finite
// values and multiply zero-padded image rows (see attn_fwd_small_kernel);
// tiles are zero-initialized once so causal-masked entries (never written)
// contribute exact zeros.
// ---------------------------------------------------------------------------

template <bool CAUSAL>
__global__ __launch_bounds__(320) void attn_bwd_small_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ dO, const float* __restrict__ lse, bf16* __restrict__ dq,
    bf16* __restrict__ dk, bf16* __restrict__ dv, int Lq, int Lk, float scale, int H,
    hstride q_s, hstride k_s, hstride v_s, hstride do_s, hstride dq_s, hstride dk_s,
    hstride dv_s) {
  constexpr int D = 64;
  constexpr int LP = 96;         // image rows (three 32-row blocks)
  constexpr int TP = 88;         // tile pitch
  constexpr int IMG = LP * D;    // shorts per image
  constexpr int TILE = 80 * TP;  // shorts per tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* imgA = reinterpret_cast<short*>(smem);  // K image
  short* imgQ = imgA + IMG;                      // Q image (ph2)
  short* imgD = imgQ + IMG;                      // dO image (ph2)
  short* PT = imgD + IMG;                        // P^T  [key][q]
  short* DST = PT + TILE;                        // dS^T [key][q]
  short* DSQ = DST + TILE;                       // dS   [q][key] (+8 zeroed pad after)

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int lo = lane & 15, hi = lane >> 4;
  const int64_t bh = blockIdx.x;
  const bf16* qp = head_ptr(q, q_s, bh, H);
  const bf16* kp = head_ptr(k, k_s, bh, H);
  const bf16* vp = head_ptr(v, v_s, bh, H);
  const bf16* dop = head_ptr(dO, do_s, bh, H);
  bf16* dqp = head_ptr(dq, dq_s, bh, H);
  bf16* dkp = head_ptr(dk, dk_s, bh, H);
  bf16* dvp = head_ptr(dv, dv_s, bh, H);

  // zero the tiles + pad once (masked entries are never written)
  for (int i = threadIdx.x; i < (3 * TILE + 8) / 8; i += 320)
    *reinterpret_cast<bf16x8*>(PT + i * 8) = bf16x8{};
  auto stage = [&](short* img, const bf16* src, int64_t sl, int rows) {
    for (int idx = (int)threadIdx.x; idx < IMG / 8; idx += 320) {
      const int row = idx >> 3, d8 = (idx & 7) * 8;
      bf16x8 vv{};
      if (row < rows) vv = *reinterpret_cast<const bf16x8*>(src + (int64_t)row * sl + d8);
      *reinterpret_cast<bf16x8*>(img + boff<D>(row, d8)) = vv;
    }
  };
  stage(imgA, kp, k_s.l, Lk);
  stage(imgQ, qp, q_s.l, Lq);
  stage(imgD, dop, do_s.l, Lq);
  const int nq = (Lq + 15) / 16;
  const int nkt = (Lk + 15) / 16;
  __syncthreads();

  // ---- phase 1: per q-strip --------------------------------------------
  if (wave < nq) {
    const int qs = wave;
    const int q0 = 16 * qs;
    const int ktmax = CAUSAL ? min(nkt, qs + 1) : nkt;
    bf16x8 kfr[5][2], vfr[5][2];
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
      const int key = 16 * kt + lo;
      const bool ok = kt < ktmax && key < Lk;
#pragma unroll
      for (int sj = 0; sj < 2; ++sj) {
        kfr[kt][sj] = ok ? *reinterpret_cast<const bf16x8*>(
                               kp + (int64_t)key * k_s.l + 32 * sj + hi * 8)
                         : bf16x8{};
        vfr[kt][sj] = ok ? *reinterpret_cast<const bf16x8*>(
                               vp + (int64_t)key * v_s.l + 32 * sj + hi * 8)
                         : bf16x8{};
      }
    }
    const int qrow = min(q0 + lo, Lq - 1);
    const bf16x8 qb0 = *reinterpret_cast<const bf16x8*>(qp + (int64_t)qrow * q_s.l + hi * 8);
    const bf16x8 qb1 =
        *reinterpret_cast<const bf16x8*>(qp + (int64_t)qrow * q_s.l + 32 + hi * 8);
    const bf16x8 db0 =
        *reinterpret_cast<const bf16x8*>(dop + (int64_t)qrow * do_s.l + hi * 8);
    const bf16x8 db1 =
        *reinterpret_cast<const bf16x8*>(dop + (int64_t)qrow * do_s.l + 32 + hi * 8);
    f32x4 sc[5] = {}, dpc[5] = {};
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
      if (kt >= ktmax) continue;
      sc[kt] = MFMA16(kfr[kt][0], qb0, sc[kt]);
      sc[kt] = MFMA16(kfr[kt][1], qb1, sc[kt]);
      dpc[kt] = MFMA16(vfr[kt][0], db0, dpc[kt]);
      dpc[kt] = MFMA16(vfr[kt][1], db1, dpc[kt]);
    }
    __builtin_amdgcn_s_setprio(0);
    const int q_idx = q0 + lo;
    const float lse_q = lse[bh * Lq + qrow];
    float pv[20];
    float dsum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * kt + 4 * hi + r;
        const bool ok =
            kt < ktmax && key < Lk && q_idx < Lq && (!CAUSAL || key <= q_idx);
        const float p = ok ? __expf(sc[kt][r] * scale - lse_q) : 0.f;
        pv[4 * kt + r] = p;
        dsum += p * dpc[kt][r];
      }
    }
    dsum += __shfl_xor(dsum, 16, WAVE);
    dsum += __shfl_xor(dsum, 32, WAVE);  // delta[q] == rowsum(dO o O)
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
      bf16x4 ds4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * kt + 4 * hi + r;
        const float p = pv[4 * kt + r];
        const float ds = p * (dpc[kt][r] - dsum) * scale;
        PT[key * TP + q_idx] = f2bfs(p);
        DST[key * TP + q_idx] = f2bfs(ds);
        ds4[r] = f2bfs(ds);
      }
      *reinterpret_cast<bf16x4*>(DSQ + q_idx * TP + 16 * kt + 4 * hi) = ds4;
    }
    // dQ strip = dS @ K (B = tr fragments of the K image)
    f32x4 adq[4] = {};
    const int smax = (16 * ktmax + 31) / 32;
#pragma unroll
    for (int sb = 0; sb < 3; ++sb) {
      if (sb >= smax) continue;
      bf16x8 bfr[4];
      tr_frag_x4((lds_cp)(const void*)(imgA + sb * 32 * D) + lane * 8, bfr);
      const bf16x8 pa = row_frag(DSQ, q0 + lo, TP, sb, hi);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) adq[dt] = MFMA16(pa, bfr[dt], adq[dt]);
      __builtin_amdgcn_s_setprio(0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qr = q0 + 4 * hi + r;
      if (qr >= Lq) continue;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        dqp[(int64_t)qr * dq_s.l + 16 * dt + lo] = f2bf(adq[dt][r]);
    }
  }
  __syncthreads();  // phase-1 tile writes visible

  // ---- phase 2: per key-strip ------------------------------------------
  if (wave < nkt) {
    const int k0 = 16 * wave;
    const int smin = CAUSAL ? k0 / 32 : 0;
    const int nsq = (Lq + 31) / 32;
    f32x4 adk[4] = {}, adv[4] = {};
    for (int sb = smin; sb < nsq; ++sb) {
      bf16x8 bq[4], bd[4];
      tr_frag_x4((lds_cp)(const void*)(imgQ + sb * 32 * D) + lane * 8, bq);
      tr_frag_x4((lds_cp)(const void*)(imgD + sb * 32 * D) + lane * 8, bd);
      const bf16x8 ak = row_frag(DST, k0 + lo, TP, sb, hi);
      const bf16x8 av = row_frag(PT, k0 + lo, TP, sb, hi);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        adk[dt] = MFMA16(ak, bq[dt], adk[dt]);
        adv[dt] = MFMA16(av, bd[dt], adv[dt]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kr = k0 + 4 * hi + r;
      if (kr >= Lk) continue;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        dkp[(int64_t)kr * dk_s.l + 16 * dt + lo] = f2bf(adk[dt][r]);
        dvp[(int64_t)kr * dv_s.l + 16 * dt + lo] = f2bf(adv[dt][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Resident fused backward (Lq == Lk = L, 81 <= L <= 256, D = 64, non-causal):
// ONE kernel replaces the d2 + dkv + dq trio. One workgroup per (b, h) keeps
// a whole operand pair in LDS block images and computes BOTH orientations
// from them, so no P/dS tile is ever exchanged between waves and K, V, Q, dO
// come from HBM once (the tiled pair reads each of them twice, from two
// workgroups on different XCDs). ceil(L/32) waves, each owning the two
// 16-row strips wave and wave + nwaves; two image slots (K/V, then Q/dO), so
// LDS is 58 KiB at L = 197 and two workgroups share a CU: one loads or
// stores while the other computes.
//   phase 1 (strip = 16 queries): S^T = K.Q^T and dP^T = V.dO^T with
//     A-fragments read ds_read_b128 from the K/V images and the strip's own
//     Q/dO rows held in registers as B-fragments; keys are walked 32 at a
//     time. delta[q] = rowsum(dO o O) of the strip's own 16 rows (one sweep
//     over the keys; costs one read of O). dQ^T += K^T.dS^T with tr-read
//     fragments of the K image.
//   between the phases the wave takes its own K/V rows out of the images
//     (phase-2 B-fragments) and Q/dO (L2-hot) replace K/V in the two slots.
//   phase 2 (strip = 16 keys): S = Q.K^T and dP = dO.V^T, A-fragments from
//     the Q/dO images; dV^T += dO^T.P and dK^T += Q^T.dS with tr-read
//     fragments of the dO/Q images; lse[q] and delta[q] come from LDS.
// The second GEMM of each phase takes its dS / P operand straight from the
// accumulator registers of the first: lane (lo, hi) of two 16-row C tiles
// t = 0, 1 holds rows 16t + 4hi + r (r = 0..3) of column lo, which is a
// fragment X[lo][8hi + j] whose contraction slot 8hi + j stands for row
// 4hi + j (j < 4) or 16 + 4hi + (j - 4) of the 32-row block. The images
// therefore keep their 8 row-quads in NATURAL order (boff<> stores evens
// first, which makes slot == row): ds_read_b64_tr_b16 at base + lane*8
// fetches slot-quad sq from position (sq&1)*4 + (sq>>1), exactly the
// row-quad the permuted fragment expects. The tr-read fragment is used as
// the A operand and the P/dS fragment as B (the register contents of an A
// and a B fragment of the same matrix are identical), so the accumulators
// hold TRANSPOSED output tiles: lane = output row lo, 4 consecutive d, one
// 8-byte store per tile instead of four 2-byte ones.
// Within a 32-row x 16-d sub-block rows are 32 B apart, so the ds_read_b128
// A-fragment reads (8 contiguous d of row lo) hit 16 distinct 16-B slots per
// lane group.
// Image rows >= L are zero; every global load is clamped to row L-1, every
// store guarded by row < L; P and dS of padded rows are forced to exact 0.
// Synchronisation: barrier 1 orders the K/V staging writes (images, lse,
// zeroed delta) before every phase-1 read and before phase 1's delta
// writes. Barrier 2 retires every read of the K/V images (phase 1 and the
// phase-2 B-fragment loads) before Q/dO overwrite them, and orders phase
// 1's delta writes before phase 2's delta reads. Barrier 3 publishes the
// Q/dO images to phase 2. All three barriers and every tr read are outside
// divergent control flow (the branches around them are wave-uniform), so
// EXEC is all ones at each ds_read_b64_tr_b16.
// RES_LMIN, RES_LMAX and the image layout noff are in mfma.h (shared with the
// resident forward, attention.hip).
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(512, 4) void attn_bwd_resident_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ o, const bf16* __restrict__ dO, const float* __restrict__ lse,
    bf16* __restrict__ dq, bf16* __restrict__ dk, bf16* __restrict__ dv, int L, float scale,
    int H, hstride q_s, hstride k_s, hstride v_s, hstride o_s, hstride do_s, hstride dq_s,
    hstride dk_s, hstride dv_s) {
  constexpr int D = 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int LP = (L + 31) & ~31;  // image rows: whole 32-row blocks
  const int IMG = LP * D;
  short* imgA = reinterpret_cast<short*>(smem);  // K, then Q
  short* imgB = imgA + IMG;                      // V, then dO
  float* lse_s = reinterpret_cast<float*>(imgB + IMG);  // [LP]
  float* dl_s = lse_s + LP;                             // [LP] delta

  const int tid = threadIdx.x;
  const int nthr = blockDim.x;  // 64 * LP/32: the image has exactly 4 16-B chunks per thread
  const int nw = nthr / WAVE;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int lo = lane & 15, hi = lane >> 4;
  const int64_t bh = blockIdx.x;
  const bf16* qp = head_ptr(q, q_s, bh, H);
  const bf16* kp = head_ptr(k, k_s, bh, H);
  const bf16* vp = head_ptr(v, v_s, bh, H);
  const bf16* op = head_ptr(o, o_s, bh, H);
  const bf16* dop = head_ptr(dO, do_s, bh, H);
  const int nblk = LP / 32;

  // ---- a strip's own Q/dO rows (phase-1 B-fragments) and its delta ---------
  bf16x8 qb[2], dob[2];
  float dl;
  auto load_rows = [&](int s0) {
    const int srow = min(s0 + lo, L - 1);
    dl = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      qb[s] = *reinterpret_cast<const bf16x8*>(qp + (int64_t)srow * q_s.l + 32 * s + hi * 8);
      dob[s] = *reinterpret_cast<const bf16x8*>(dop + (int64_t)srow * do_s.l + 32 * s + hi * 8);
      const bf16x8 ov =
          *reinterpret_cast<const bf16x8*>(op + (int64_t)srow * o_s.l + 32 * s + hi * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) dl += bfs2f(dob[s][j]) * bfs2f(ov[j]);
    }
    dl += __shfl_xor(dl, 16, WAVE);
    dl += __shfl_xor(dl, 32, WAVE);  // delta[s0 + lo] = rowsum(dO o O)
  };
  load_rows(16 * wave);  // first strip

  // ---- stage K, V + lse ----------------------------------------------------
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = tid + it * nthr;
    const int row = idx >> 3, d8 = (idx & 7) * 8;
    const int rc = min(row, L - 1);
    bf16x8 kk = *reinterpret_cast<const bf16x8*>(kp + (int64_t)rc * k_s.l + d8);
    bf16x8 vv = *reinterpret_cast<const bf16x8*>(vp + (int64_t)rc * v_s.l + d8);
    if (row >= L) kk = vv = bf16x8{};
    const int off = noff(row, d8);
    *reinterpret_cast<bf16x8*>(imgA + off) = kk;
    *reinterpret_cast<bf16x8*>(imgB + off) = vv;
  }
  for (int i = tid; i < LP; i += nthr) {
    lse_s[i] = i < L ? lse[bh * L + i] : 0.f;
    dl_s[i] = 0.f;
  }
  __syncthreads();  // barrier 1

  // ---- phase 1: wave = query strips wave, wave + nw -----------------------
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int s0 = 16 * (wave + i * nw);
    if (s0 >= L) continue;  // wave-uniform
    if (i == 1) load_rows(s0);
    const bool sok = s0 + lo < L;
    const float lse_q = lse_s[min(s0 + lo, L - 1)];
    const float dli = dl;
    if (hi == 0) dl_s[s0 + lo] = dli;
    f32x4 adq[4] = {};
    for (int kb = 0; kb < nblk; ++kb) {
      f32x4 sc[2] = {}, dpc[2] = {};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (32 * kb + 16 * t >= L) continue;  // whole 16-key tile is padding (wave-uniform)
        bf16x8 ka[2], va[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int off = noff(32 * kb + 16 * t + lo, 32 * s + hi * 8);
          ka[s] = *reinterpret_cast<const bf16x8*>(imgA + off);
          va[s] = *reinterpret_cast<const bf16x8*>(imgB + off);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          sc[t] = MFMA16(ka[s], qb[s], sc[t]);
          dpc[t] = MFMA16(va[s], dob[s], dpc[t]);
        }
        __builtin_amdgcn_s_setprio(0);
      }
      bf16x8 dsa;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = 32 * kb + 16 * t + 4 * hi + r;
          const bool ok = sok && key < L;
          const float p = ok ? __expf(sc[t][r] * scale - lse_q) : 0.f;
          const float ds = ok ? p * (dpc[t][r] - dli) * scale : 0.f;
          dsa[4 * t + r] = f2bfs(ds);
        }
      }
      bf16x8 bfr[4];
      tr_frag_x4((lds_cp)(const void*)(imgA + kb * 32 * D) + lane * 8, bfr);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) adq[dt] = MFMA16(bfr[dt], dsa, adq[dt]);
      __builtin_amdgcn_s_setprio(0);
    }
    // adq holds dQ^T tiles: lane = query lo, d = 16dt + 4hi + r -> 8-byte stores
    if (sok) {
      bf16* dqp = head_ptr(dq, dq_s, bh, H) + (int64_t)(s0 + lo) * dq_s.l + 4 * hi;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        bf16x4 pk;
#pragma unroll
        for (int r = 0; r < 4; ++r) pk[r] = f2bfs(adq[dt][r]);
        *reinterpret_cast<bf16x4*>(dqp + 16 * dt) = pk;
      }
    }
  }

  // ---- between the phases: Q/dO replace K/V in the two image slots --------
  bf16x8 qst[4], dst[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = tid + it * nthr;
    const int row = idx >> 3, d8 = (idx & 7) * 8;
    const int rc = min(row, L - 1);
    qst[it] = *reinterpret_cast<const bf16x8*>(qp + (int64_t)rc * q_s.l + d8);
    dst[it] = *reinterpret_cast<const bf16x8*>(dop + (int64_t)rc * do_s.l + d8);
    if (row >= L) qst[it] = dst[it] = bf16x8{};
  }
  // own K/V rows of the two key strips as phase-2 B-fragments, taken from
  // the images before they are overwritten (image rows >= L are zero)
  bf16x8 kbf[2][2], vbf[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int srow = min(16 * (wave + i * nw) + lo, LP - 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int off = noff(srow, 32 * s + hi * 8);
      kbf[i][s] = *reinterpret_cast<const bf16x8*>(imgA + off);
      vbf[i][s] = *reinterpret_cast<const bf16x8*>(imgB + off);
    }
  }
  __syncthreads();  // barrier 2: K/V images retired, every strip's delta in LDS
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = tid + it * nthr;
    const int off = noff(idx >> 3, (idx & 7) * 8);
    *reinterpret_cast<bf16x8*>(imgA + off) = qst[it];
    *reinterpret_cast<bf16x8*>(imgB + off) = dst[it];
  }
  __syncthreads();  // barrier 3: Q/dO images published

  // ---- phase 2: wave = key strips wave, wave + nw --------------------------
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int s0 = 16 * (wave + i * nw);
    if (s0 >= L) continue;  // wave-uniform
    const bool sok = s0 + lo < L;
    f32x4 adk[4] = {}, adv[4] = {};
    for (int qblk = 0; qblk < nblk; ++qblk) {
      f32x4 sc[2] = {}, dpc[2] = {};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (32 * qblk + 16 * t >= L) continue;  // whole 16-query tile is padding
        bf16x8 qa[2], da[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int off = noff(32 * qblk + 16 * t + lo, 32 * s + hi * 8);
          qa[s] = *reinterpret_cast<const bf16x8*>(imgA + off);
          da[s] = *reinterpret_cast<const bf16x8*>(imgB + off);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          sc[t] = MFMA16(qa[s], kbf[i][s], sc[t]);
          dpc[t] = MFMA16(da[s], vbf[i][s], dpc[t]);
        }
        __builtin_amdgcn_s_setprio(0);
      }
      bf16x8 pa, dsa;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int qi0 = 32 * qblk + 16 * t + 4 * hi;
        const f32x4 ls4 = *reinterpret_cast<const f32x4*>(lse_s + qi0);
        const f32x4 dl4 = *reinterpret_cast<const f32x4*>(dl_s + qi0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = sok && qi0 + r < L;
          const float p = ok ? __expf(sc[t][r] * scale - ls4[r]) : 0.f;
          const float ds = ok ? p * (dpc[t][r] - dl4[r]) * scale : 0.f;
          pa[4 * t + r] = f2bfs(p);
          dsa[4 * t + r] = f2bfs(ds);
        }
      }
      bf16x8 bfr[4];  // one fragment set at a time (register budget)
      tr_frag_x4((lds_cp)(const void*)(imgB + qblk * 32 * D) + lane * 8, bfr);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) adv[dt] = MFMA16(bfr[dt], pa, adv[dt]);
      __builtin_amdgcn_s_setprio(0);
      tr_frag_x4((lds_cp)(const void*)(imgA + qblk * 32 * D) + lane * 8, bfr);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) adk[dt] = MFMA16(bfr[dt], dsa, adk[dt]);
      __builtin_amdgcn_s_setprio(0);
    }
    // transposed tiles again: lane = key lo, d = 16dt + 4hi + r
    if (sok) {
      bf16* dkp = head_ptr(dk, dk_s, bh, H) + (int64_t)(s0 + lo) * dk_s.l + 4 * hi;
      bf16* dvp = head_ptr(dv, dv_s, bh, H) + (int64_t)(s0 + lo) * dv_s.l + 4 * hi;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        bf16x4 pk, pv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pk[r] = f2bfs(adk[dt][r]);
          pv[r] = f2bfs(adv[dt][r]);
        }
        *reinterpret_cast<bf16x4*>(dkp + 16 * dt) = pk;
        *reinterpret_cast<bf16x4*>(dvp + 16 * dt) = pv;
      }
    }
  }
}

}  // namespace

void attn_bwd_fused(torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor o,
                    torch::Tensor dO, torch::Tensor lse, torch::Tensor dq, torch::Tensor dk,
                    torch::Tensor dv, bool causal, double scale, std::string path) {
  // all tensors (B,H,L,D) views, innermost contiguous, arbitrary b/h/l strides
  check_attn_args("attn_bwd_fused", {{"q", q}, {"o", o}, {"dO", dO}, {"dq", dq}},
                  {{"k", k}, {"v", v}, {"dk", dk}, {"dv", dv}}, &lse);
  const int Dr = q.size(3);
  const int DP = Dr <= 64 ? 64 : (Dr <= 96 ? 96 : 128);
  const int B = q.size(0), H = q.size(1), Lq = q.size(2), Lk = k.size(2);
  const unsigned BH = (unsigned)((int64_t)B * H);
  auto stream = at::hip::getCurrentHIPStream();

  // path: "auto" picks small (L <= 80) / resident (81..RES_LMAX) / tiled;
  // "tiled" forces d2 + dkv + dq; "resident" fails outside its domain
  TORCH_CHECK(path == "auto" || path == "tiled" || path == "resident",
              "attn_bwd_fused: path must be auto, tiled or resident, got ", path);
  const bool aligned = res_aligned({&q, &k, &v, &o, &dO, &dq, &dk, &dv});
  const bool resident_ok = Dr == 64 && Lq == Lk && !causal && Lk >= RES_LMIN &&
                           Lk <= RES_LMAX && aligned;
  TORCH_CHECK(path != "resident" || resident_ok,
              "attn_bwd_fused: path=resident needs D == 64, Lq == Lk, non-causal, ",
              RES_LMIN, " <= L <= ", RES_LMAX, " and 16-byte aligned rows; got D=", Dr,
              " Lq=", Lq, " Lk=", Lk, " causal=", causal, " aligned=", aligned);
  if (path != "tiled" && resident_ok) {
    // one wave per 32 rows (two 16-row strips each); two images + lse + delta
    const int LP = (Lk + 31) & ~31;
    const size_t rshmem = (size_t)2 * LP * 64 * sizeof(short) + (size_t)2 * LP * sizeof(float);
    // the LDS limit is raised once, to the largest supported L
    constexpr size_t rshmem_max =
        (size_t)2 * RES_LMAX * 64 * sizeof(short) + (size_t)2 * RES_LMAX * sizeof(float);
    launch_lds<attn_bwd_resident_kernel>(
        dim3(BH), dim3(LP / 32 * WAVE), rshmem, rshmem_max, stream, bf16_ptr(q), bf16_ptr(k),
        bf16_ptr(v), bf16_ptr(o), bf16_ptr(dO), lse.data_ptr<float>(), bf16_ptr(dq),
        bf16_ptr(dk), bf16_ptr(dv), Lk, (float)scale, H, hstrides(q), hstrides(k), hstrides(v),
        hstrides(o), hstrides(dO), hstrides(dq), hstrides(dk), hstrides(dv));
    return;
  }

  // small-L fused path: one kernel, no delta buffer (Lq == Lk <= 80, D = 64)
  if (path != "tiled" && Dr == 64 && Lq == Lk && Lk <= 80) {
    const size_t shmem = (3 * 96 * 64 + 3 * 80 * 88 + 8) * sizeof(short);
    with_flags(
        [&](auto c) {
          launch_lds<attn_bwd_small_kernel<decltype(c)::value>>(
              dim3(BH), dim3(320), shmem, shmem, stream, bf16_ptr(q), bf16_ptr(k), bf16_ptr(v),
              bf16_ptr(dO), lse.data_ptr<float>(), bf16_ptr(dq), bf16_ptr(dk), bf16_ptr(dv), Lq,
              Lk, (float)scale, H, hstrides(q), hstrides(k), hstrides(v), hstrides(dO),
              hstrides(dq), hstrides(dk), hstrides(dv));
        },
        causal);
    return;
  }

  // D = rowsum(dO * O)
  auto Dv = torch::empty({(int64_t)B * H * Lq}, q.options().dtype(torch::kFloat32));
  {
    const int64_t nrows = (int64_t)B * H * Lq;
    const dim3 grid((unsigned)std::min<int64_t>((nrows + 3) / 4, 4096));
    hipLaunchKernelGGL(attn_d2_kernel, grid, dim3(256), 0, stream, bf16_ptr(dO), bf16_ptr(o),
                       Dv.data_ptr<float>(), H, Lq, Dr, nrows, hstrides(dO), hstrides(o));
  }

  const int pitch = DP + 8;
  const size_t shmem_dkv =
      (2 * (2 * BLK * DP + 2 * BLK * pitch) + 4 * 16 * pitch) * sizeof(short);
  const size_t shmem_dq = (2 * (BLK * DP + 2 * BLK * pitch) + 4 * 16 * pitch) * sizeof(short);
  const int ntk = (Lk + BLK - 1) / BLK;
  const int ntq = (Lq + BLK - 1) / BLK;
  const int tpw = tiles_per_wg(DP);
  with_flags(
      [&](auto c) {
        with_int<64, 96, 128>(DP, "padded head dim", [&](auto dp) {
          constexpr bool C = decltype(c)::value;
          constexpr int P = decltype(dp)::value;
          launch_lds<attn_bwd_dkv_kernel<C, P>>(
              dim3((ntk + tpw - 1) / tpw, BH), dim3(256), shmem_dkv, shmem_dkv, stream,
              bf16_ptr(q), bf16_ptr(k), bf16_ptr(v), bf16_ptr(dO), lse.data_ptr<float>(),
              Dv.data_ptr<float>(), bf16_ptr(dk), bf16_ptr(dv), Lq, Lk, (float)scale, H, Dr,
              hstrides(q), hstrides(k), hstrides(v), hstrides(dO), hstrides(dk), hstrides(dv));
          launch_lds<attn_bwd_dq_kernel<C, P>>(
              dim3((ntq + tpw - 1) / tpw, BH), dim3(256), shmem_dq, shmem_dq, stream,
              bf16_ptr(q), bf16_ptr(k), bf16_ptr(v), bf16_ptr(dO), lse.data_ptr<float>(),
              Dv.data_ptr<float>(), bf16_ptr(dq), Lq, Lk, (float)scale, H, Dr, hstrides(q),
              hstrides(k), hstrides(v), hstrides(dO), hstrides(dq));
        });
      },
      causal);
}
