// The body of the decode kernels: included INTO attn_i8_decode_paged_kernel and attn_i8_decode_paged_v4_kernel
// (sage_attn_decode.hip, which says what it does) and attn_i8_decode_paged_window_kernel (sage_attn_decode_window.hip), not a
// header in the usual sense.
// Expects in scope: the kernel parameter block `p` and the compile-time constants D, KTHREAD, V_BF16, PV_FP8, PV_FP4
// (PV_FP4, with PV_FP8, whose P it shares: V is the paged MXFP4 image, held in registers).  What the windowed kernel adds stands
// under SAGE_ATTN_DECODE_BODY_WINDOW, which its file defines: the other kernels keep their text.
#ifndef SAGE_ATTN_DECODE_BODY_OF_KERNEL
#error "sage_attn_decode_body.h is the body of the decode kernels (sage_attn_decode*.hip): included nowhere else"
#endif
  static_assert(!(PV_FP8 && V_BF16), "fp8 V has no bf16 flavour");
  static_assert(!PV_FP4 || PV_FP8, "the FP4 image is multiplied by the FP8 mode's P");
  constexpr int KS = D / 32;                        // k-steps of the int8 QK^T MFMA
  constexpr int DT = D / 32;                        // 32-wide d tiles of O^T
  constexpr int KBYTES = 64 * D;                    // one K tile (int8)
  constexpr int VBYTES = PV_FP8 ? 64 * D : 128 * D; // one V tile: e4m3 [D][64] or 16-bit [64][D]
  constexpr int KCH = D / 16;                       // 16-byte chunks per K row
  constexpr int VCH = PV_FP8 ? 4 : D / 8;           // ... per row of the V image
  constexpr int VROWS = PV_FP8 ? D : 64;
  constexpr int NK = 64 * KCH / 64, NV = VROWS * VCH / 64;  // copies of 64 x 16 bytes per tile
  // the wave's vector-memory operations per tile behind the K copies: the V copies, or (PV_FP4) DT fragment loads and one scale load
  constexpr int NVM = PV_FP4 ? DT + 1 : NV;
  static_assert(kDecodeRing * (NK + NVM) < 64, "the counted waits: vmcnt is a 6-bit counter");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const k_lds = smem;
  char* const v_lds = smem + kDecodeRing * KBYTES;

  // ---- block -> (b, h, split), XCD aware: the splits of a head are neighbours, then the batches of a head
  const int nwg = gridDim.x;
  int lid;
  {
    const int orig = blockIdx.x, xcd = orig & 7, qq = nwg >> 3, rr = nwg & 7;
    lid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (orig >> 3);
  }
  const int split = lid % p.num_splits;
  const int bh = lid / p.num_splits;
  const int h = bh / p.B, b = bh % p.B;
  const int hk = h / (p.Hq / p.Hk);
  const int M_ = p.M;

  // ---- the split's range of logical tiles and the diagonal in its coordinates (wave uniform; an empty split returns at once)
  const int len_b = min(max(uniform_load_i32(p.kv_lens + b), 0), p.N);
#ifdef SAGE_ATTN_DECODE_BODY_WINDOW
  // WINDOW (attn_i8_decode_paged_window_kernel, sage_attn_decode_window.hip, which defines the macro, the int `dw_window` >= 1,
  // `dw_sinks` and `dw_fused`; the rule: include/sageattn_hip_decode_window.h).  The call is one q-block: its keys lie between
  // the lower limit of row 0 and the upper limit of the last row < M, the tiles [dw_tlo, dw_tlo + dw_nt), cut into the splits'
  // ranges like the batch's tiles otherwise.  No tile below dw_tlo is named from here on, so no table entry below
  // max(off_b - window + 1, 0) / page_size is read.  (window <= p.N: the host clamps it.)  dw_fused -- the host sets it iff
  // num_splits == 1 -- finishes the rows in this launch (the epilogue below); a sequence without keys then gets its zeros and
  // -inf here, from the lanes that own its rows.
  auto dw_store_empty = [&]() __attribute__((always_inline)) {
    const int row = threadIdx.x & 31, hh = threadIdx.x >> 5;
    if (row >= M_) return;
    uint16_t* const op = p.o + b * p.osb + h * p.osh + (int64_t)row * p.osn + 4 * hh;
#pragma unroll
    for (int d0 = 0; d0 < D; d0 += 8) *reinterpret_cast<uint2*>(op + d0) = make_uint2(0u, 0u);
    if (hh == 0 && p.lse) p.lse[((int64_t)b * p.Hq + h) * M_ + row] = -INFINITY;
  };
  const int dw_off = len_b - M_ / p.q_fold;
  const int dw_lo = max(dw_off - dw_window + 1, 0);
  const int dw_hi = min((M_ - 1) / p.q_fold + dw_off, len_b - 1);
  if (dw_hi < 0) {
    if (dw_fused) dw_store_empty();
    return;
  }
  const int dw_tlo = dw_lo >> 6, dw_nt = (dw_hi >> 6) - dw_tlo + 1, tps_b = (dw_nt + p.num_splits - 1) / p.num_splits;
  const int sk_t0 = dw_tlo + split * tps_b;
  const int t1 = min(sk_t0 + tps_b, dw_tlo + dw_nt);
#else
  const int ntk_b = (len_b + 63) >> 6, tps_b = (ntk_b + p.num_splits - 1) / p.num_splits;
  const int sk_t0 = split * tps_b;
  const int t1 = min(sk_t0 + tps_b, ntk_b);
#endif
  if (sk_t0 >= t1) return;
  const int N_ = min(len_b, t1 << 6) - (sk_t0 << 6);         // keys from the split's first one to its end
  const int sk_off = (len_b - (sk_t0 << 6)) - M_ / p.q_fold;  // off_b in the split's coordinates
  const int sk_end = (M_ - 1) / p.q_fold + sk_off + 1;        // key bound of the last row < M
  if (sk_end <= 0) return;
  const int ntiles = (min(N_, sk_end) + 63) >> 6;
  const int last_tile = ntiles - 1;
  // tiles [0, n_plain) need no mask: they end before the sequence does and at or before the limit of row 0
  int n_plain = ntiles;
  if (N_ & 63) n_plain = min(n_plain, N_ >> 6);
  n_plain = min(n_plain, (max(sk_off, -1) + 1) >> 6);

  const int lane = threadIdx.x;
  const int r = lane & 31, hh = lane >> 5;
  const int row = r;
  const int rowc = min(row, M_ - 1);
  // the last key (of the split's coordinates) the lane's row may attend; every negative limit is held at -1
  const int lim_l = max(row / p.q_fold + sk_off, -1);
#ifdef SAGE_ATTN_DECODE_BODY_WINDOW
  // The FIRST key the lane's row may attend is lim_l - window + 1: no register of its own, mask_limit forms it from lim_l where
  // a tile needs it (a row whose lim_l is held at -1 has no key whatever its lower limit is; rows >= M keep the limits of their
  // row index on both sides).  dw_nlm, the tiles that need the lower mask, counted once: tile j does iff 64 * j < the lower limit
  // of the last row < M -- the first one or two tiles of the first split that runs.
  const int dw_nlm = (max((M_ - 1) / p.q_fold + sk_off - dw_window + 1, 0) + 63) >> 6;
#define SAGE_DECODE_TILE_MASKED(t) ((t) >= n_plain || (t) < dw_nlm)
#else
#define SAGE_DECODE_TILE_MASKED(t) ((t) >= n_plain)
#endif

  // ---- Q^T fragments (B operand) and the row's scale: the fused Q quantizer of the shared body on the wave's 32 rows.  Lane
  //      (r, hh) owns the 16-column chunks [32 * ks + 16 * hh, +16) of its row; rows >= M load the last row's bytes and are zeros.
  v4i qf[KS];
  float qsc;
#ifdef SAGE_ATTN_DECODE_BODY_WINDOW
  float dw_corr = 0.f;  // q . km of the lane's row, held for the finish inside the launch
#endif
  auto prepare_q = [&]() __attribute__((always_inline)) {
    const bool valid = row < M_;
    const uint16_t* qp = p.q_f16 + b * p.qsb + h * p.qsh + (int64_t)rowc * p.qsn + 16 * hh;
    uint4 raw[KS][2];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      raw[ks][0] = *reinterpret_cast<const uint4*>(qp + 32 * ks);
      raw[ks][1] = *reinterpret_cast<const uint4*>(qp + 32 * ks + 8);
    }
    // the LSE correction q . k_mean: computed and parked in the caller's LSE slot by split 0 only; the merge consumes it
    const uint16_t* kmp = (p.km && p.lse && split == 0) ? p.km + ((int64_t)b * p.Hk + hk) * D + 16 * hh : nullptr;
    auto fused_q = [&](auto bf16_tag) __attribute__((always_inline)) {
      constexpr bool QBF = decltype(bf16_tag)::value;
      if (!valid) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) raw[ks][0] = raw[ks][1] = make_uint4(0u, 0u, 0u, 0u);
      }
      float amax = 0.f, dot = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          float f[8];
          unpack8<QBF>(raw[ks][c], f);
#pragma unroll
          for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
          if (kmp) {
            float g[8];
            const uint4 uk = *reinterpret_cast<const uint4*>(kmp + 32 * ks + 8 * c);
            unpack8<QBF>(uk, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) dot += f[e] * g[e];
          }
        }
      amax = swap_max(amax);  // the other half of the row
      const float lse_corr = swap_sum(dot);
#ifdef SAGE_ATTN_DECODE_BODY_WINDOW
      dw_corr = lse_corr;  // (dw_fused: the epilogue adds it itself, nothing is parked)
      if (!dw_fused && split == 0 && p.lse && hh == 0 && valid) p.lse[((int64_t)b * p.Hq + h) * M_ + row] = lse_corr;
#else
      if (split == 0 && p.lse && hh == 0 && valid) p.lse[((int64_t)b * p.Hq + h) * M_ + row] = lse_corr;
#endif
      if constexpr (KTHREAD) {  // per thread: rows with equal r % 8 of the 32-row block share a scale
        amax = fmaxf(amax, __shfl_xor(amax, 8));
        amax = fmaxf(amax, __shfl_xor(amax, 16));
      } else {                  // per warp: warpq rows (16 or 32) share a scale
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
        if (p.warpq == 32) amax = fmaxf(amax, __shfl_xor(amax, 16));
      }
      const float a_c = fmaxf(amax, 0.0000001f);
      const float sc = KTHREAD ? amax / 127.f + 0.0000001f : a_c / 127.f;
      const float inv = 127.f / a_c;
      const float rcp_sc = 1.0f / sc;
      const bool rcp_bad = !(fabsf(rcp_sc) < 3.0e38f);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        uint32_t w[4];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          float f[8];
          unpack8<QBF>(raw[ks][c], f);
          int qv[8];
          if constexpr (KTHREAD) {
            // x / sc correctly rounded before the half-away rounding: the reciprocal product unless a value of the wave's chunk
            // lands near a rounding boundary, then the exact division decides for that chunk
            bool near = false;
#pragma unroll
            for (int e = 0; e < 8; ++e) qv[e] = round_half_away_fast(f[e] * rcp_sc, near);
            if (__builtin_amdgcn_ballot_w64(near || rcp_bad) != 0) {
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                float y = f[e] / sc;
                y = y + (y >= 0.f ? 0.5f : -0.5f);
                qv[e] = min(max((int)y, -128), 127);
              }
            }
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) qv[e] = (int)rintf(f[e] * inv);
          }
          w[2 * c] = pack_i8x4(qv[0], qv[1], qv[2], qv[3]);
          w[2 * c + 1] = pack_i8x4(qv[4], qv[5], qv[6], qv[7]);
        }
        qf[ks][0] = (int)w[0]; qf[ks][1] = (int)w[1]; qf[ks][2] = (int)w[2]; qf[ks][3] = (int)w[3];
      }
      qsc = sc * p.logit_mult;
    };
    if (p.q_bf16) fused_q(std::true_type{}); else fused_q(std::false_type{});
  };

  // ---- staging (pool -> LDS by LDS-DMA).  A wave instruction writes 64 x 16 bytes of LDS linearly, so the bank swizzle of
  //      the tile image is applied to the per-lane SOURCE offset: copy i of a tile moves the chunks 64 * i + lane.
  int k_voff[NK], v_voff[NV];
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    const int c = lane + 64 * i, kr = c / KCH, pos = c % KCH;
    k_voff[i] = kr * (int)p.ksn + ((pos ^ k_swz<D>(kr)) << 4);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i, vr = c / VCH, pos = c % VCH;
    if constexpr (PV_FP8) {
      v_voff[i] = vr * (int)p.vsn + ((pos ^ ((vr >> 2) & 3)) << 4);  // V^T row vr (= channel)
    } else {
      const int cc = (((pos >> 2) ^ v_win_swz<D>(vr)) << 2) | (pos & 3);
      v_voff[i] = (vr * (int)p.vsn + cc * 8) * 2;
    }
  }
  // Tile j of the split is logical tile sk_t0 + j of the batch: tile (sk_t0 + j) % tpp of the page that entry (sk_t0 + j) / tpp
  // of the batch's table row names.  Its descriptor: words 0-1 the 64-bit address pool + page * page stride + hk * head stride
  // + tile * tile bytes, word 2 the bytes of the tile -- of the batch's last tile those up to row len_b - 1, so the rows behind
  // it reach the LDS as zeros.  Only a tile's own bytes go through a 32-bit offset.
  const int8_t* const pg_k = p.k + hk * p.ksh;
  const uint8_t* const pg_v = p.v + hk * p.vsh * (PV_FP8 ? 1 : 2);
  const float* const pg_ks = p.k_scale + hk * p.ks_h;
  const int* const pg_row = p.block_table + (int64_t)b * p.bt_stride;
  const int pg_tmask = (1 << p.bt_shift) - 1;
  const int last_t = (N_ - 1) >> 6, last_r = (N_ - 1) & 63;
  const unsigned pg_kfull = (unsigned)(63 * (int)p.ksn + D), pg_klast = (unsigned)(last_r * (int)p.ksn + D);
  const unsigned pg_vfull = PV_FP8 ? (unsigned)((D - 1) * (int)p.vsn + 64) : (unsigned)((63 * (int)p.vsn + D) * 2);
  const unsigned pg_vlast = PV_FP8 ? pg_vfull : (unsigned)((last_r * (int)p.vsn + D) * 2);
  // the page of the tile at position `pos`, clamped to the range's last tile: no entry at or beyond ceil(len_b / page_size) is read
  auto page_at = [&](const int pos) __attribute__((always_inline)) -> int {
    return uniform_load_i32(pg_row + ((sk_t0 + min(pos, last_tile)) >> p.bt_shift));
  };
  auto dma_k = [&](const int j, const int slot, const int page) __attribute__((always_inline)) {
    const uint64_t base = reinterpret_cast<uint64_t>(pg_k) + (uint64_t)((int64_t)page * p.ksb) +
                          (uint64_t)(((sk_t0 + j) & pg_tmask) * p.k_tile_bytes);
    const v4i rs = make_rsrc_uniform(base, j == last_t ? pg_klast : pg_kfull);
    // (the LDS offset as ONE running scalar: as known constants hipcc keeps every copy's offset of every slot in a register
    //  of its own for the whole loop, and the scalar file overflows into VCC)
    unsigned off = (unsigned)(slot * KBYTES);
    asm volatile("" : "+s"(off));
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      lds_dma16_fresh(rs, off, k_voff[i], 0);
      off += 1024;
    }
  };
  auto dma_v = [&](const int j, const int slot, const int page) __attribute__((always_inline)) {
    const uint64_t base = reinterpret_cast<uint64_t>(pg_v) + (uint64_t)((int64_t)page * p.vsb * (PV_FP8 ? 1 : 2)) +
                          (uint64_t)(((sk_t0 + j) & pg_tmask) * p.v_tile_bytes);
    const v4i rs = make_rsrc_uniform(base, j == last_t ? pg_vlast : pg_vfull);
    unsigned off = (unsigned)(kDecodeRing * KBYTES + slot * VBYTES);
    asm volatile("" : "+s"(off));
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      lds_dma16_fresh(rs, off, v_voff[i], 0);
      off += 1024;
    }
  };

  // PV_FP4: V(j) -> registers, straight from the pools.  Tile base = image pool + page * page stride + hk * head stride
  // + (tile in page) * 32, a 64-bit scalar; channel block dt adds 32 channel rows to it on the scalar unit, and the lane adds
  // r * channel stride + 16 * hh: only a (page, head) slice goes through 32 bits.  The scale word: the body's load_vscale, at
  // lane * D / 32 of the tile's 2 * D bytes of the scale pool [P,Hk,tpp,2*D].  All of it from inline asm, or hipcc would wait
  // for the loads with vmcnt(0) and drain the K copies in flight; the registers are tied to the counted wait that covers them
  // by v4_landed.  A whole tile of a named page is read: the ragged one relies on the zero nibbles the append wrote.
  // ONE stage, loaded behind the last P.V MFMA of the tile before, as the body loads its scale word: with a second stage the
  // two sets trade places over the loop's back edge, and hipcc moved the set in flight from one to the other with v_mov
  // instructions in front of the wait that covers it -- it cannot know that the registers are still being written.
  v4i vfr[DT];
  int vsc = 0;
  if constexpr (PV_FP4) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) vfr[dt] = v4i{0, 0, 0, 0};
  }
  const int vf_lane = PV_FP4 ? r * (int)p.vsn + 16 * hh : 0;
  const int vs_lane = PV_FP4 ? lane * (D / 32) : 0;
  const uint8_t* const vs_head =
      PV_FP4 ? reinterpret_cast<const uint8_t*>(p.v_scale) + (int64_t)hk * ((2 * D) << p.bt_shift) : nullptr;
  (void)vfr; (void)vsc; (void)vf_lane; (void)vs_lane; (void)vs_head;
  auto load_v4 = [&](v4i (&fr)[DT], int& sc, const int j, const int page) __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int tile = (sk_t0 + j) & pg_tmask;
    const uint8_t* const tp = pg_v + (int64_t)page * p.vsb + tile * p.v_tile_bytes;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const uint8_t* const cp = tp + (int64_t)(32 * dt) * p.vsn;
      asm volatile("global_load_dwordx4 %0, %1, %2" : "+v"(fr[dt]) : "v"(vf_lane), "s"(cp) : "memory");
    }
    const uint8_t* const sp = vs_head + (int64_t)page * ((int64_t)p.Hk * ((2 * D) << p.bt_shift)) + tile * (2 * D);
    if constexpr (D == 128) asm volatile("global_load_dword %0, %1, %2" : "+v"(sc) : "v"(vs_lane), "s"(sp) : "memory");
    else asm volatile("global_load_ushort %0, %1, %2" : "+v"(sc) : "v"(vs_lane), "s"(sp) : "memory");
#endif
  };
  // behind the counted wait that covers them: the fragments and the scale word hold the tile whose P.V comes next
  auto v4_landed = [&]() __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (PV_FP4 && DT == 4)
      asm volatile("" : "+v"(vfr[0]), "+v"(vfr[1]), "+v"(vfr[2]), "+v"(vfr[3]), "+v"(vsc));
    else if constexpr (PV_FP4)
      asm volatile("" : "+v"(vfr[0]), "+v"(vfr[1]), "+v"(vsc));
#endif
  };
  // V(j) -> the registers, or slot `st` of the ring
  auto fetch_v = [&](const int j, const int st, const int page) __attribute__((always_inline)) {
    if constexpr (PV_FP4) load_v4(vfr, vsc, j, page);
    else dma_v(j, st, page);
  };
  // the P.V MFMA of channel block dt: A = e2m1 (cbsz 4; the upper four registers of the operand are not
  // live), B = e4m3, the A scale byte dt of the stage's scale word, the B scale 2^0 (pv4_mfma of sage_attn_body.h)
  auto pv4_mfma = [&](const int dt, const v8i pb, const v16f c) __attribute__((always_inline)) -> v16f {
    v8i a;
    a.s0123 = vfr[dt];
    a.s4567 = vfr[dt];
    switch (dt) {
      case 0: return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, pb, c, 4, 0, 0, vsc, 0, 0x7f7f7f7f);
      case 1: return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, pb, c, 4, 0, 1, vsc, 0, 0x7f7f7f7f);
      case 2: return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, pb, c, 4, 0, 2, vsc, 0, 0x7f7f7f7f);
      default: return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, pb, c, 4, 0, 3, vsc, 0, 0x7f7f7f7f);
    }
  };

  // ---- lane-constant LDS read addresses (slot 0; the slot is an immediate offset)
  const char* k_rd[KS];  // K A-fragment: row r (+ 32 * mt), chunk 2 * ks + hh
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) k_rd[ks] = k_lds + (r * D + (((2 * ks + hh) ^ k_swz<D>(r)) << 4));
  const char* v_rd8[2];  // fp8: V^T row r (+ 32 * dt), 16-byte chunks 2 * hh and 2 * hh + 1
#pragma unroll
  for (int c = 0; c < 2; ++c) v_rd8[c] = v_lds + (r * 64 + (((2 * hh + c) ^ ((r >> 2) & 3)) << 4));
  const char* v_rd[DT];  // 16-bit: V^T fragment by transposing read: row 4 * hh + q4 (+ 16 * quarter, + 8), window dt
  {
    const int i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3, g = (lane >> 4) & 1;
    const int rv = 4 * hh + q4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) v_rd[dt] = v_lds + (rv * (2 * D) + ((dt ^ v_win_swz<D>(rv)) << 6) + 32 * g + 8 * p4);
  }

  // ---- state
  v16f acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc_o[dt][e] = 0.f;
  float m_run = -1e30f;
  float l_run = 0.f;  // the lane's partial row sum of the unrounded p (its 32 of a tile's 64 keys)
  // FP16 P.V at head_dim 64: the row sums of the ROUNDED P on the matrix pipe, one v_mfma_f32_16x16x32_f16 per 16-key quarter
  // with a 0 / 1 selector as A: elements 0 / 1 of the accumulator hold the sums of queries l % 16 and l % 16 + 16
  constexpr bool MROW = !PV_FP8 && !V_BF16 && D == 64;
  v4f l4 = {0.f, 0.f, 0.f, 0.f};
  v8h sel8;
  {
    const _Float16 one = (((lane >> 4) & 1) == (lane & 1)) ? (_Float16)1.0f : (_Float16)0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) sel8[e] = one;
  }
  // The int32 accumulator of S^T starts at the bit pattern of 1.5 * 2^23: reinterpreted as fp32 the accumulated integer IS the
  // float 12582912 + S, so the logit needs no convert.  A masked score is the bit pattern of -inf: below every real score as an
  // integer, and exp2 of it is exactly 0.
  constexpr int kBiasI = 0x4B400000;
  constexpr float kBiasF = 12582912.0f;
  constexpr int kMaskedI = (int)0xFF800000u;
  v16i bias;
#pragma unroll
  for (int e = 0; e < 16; ++e) bias[e] = kBiasI;
  asm volatile("" : "+v"(bias));  // resident: one wave per workgroup has registers to spare

  // S^T = K . Q^T of one tile (2 x 32 keys x 32 rows) out of K slot `slot`
  auto qk = [&](const int slot, v16i (&s)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const v4i a = *reinterpret_cast<const v4i*>(k_rd[ks] + (slot * KBYTES + mt * 32 * D));
        s[mt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, qf[ks], ks == 0 ? bias : s[mt], 0, 0, 0);
      }
  };
  // dequantisation scales of a tile through the scalar cache: 4 per 64 keys (per thread) or 1, index 2 * hh + ((reg & 3) >> 1)
  float qsc_lo = 0.f, qsc_hi = 0.f;
  auto load_kscales = [&](const int j, const int page) __attribute__((always_inline)) -> float4 {
    const float* sp = pg_ks + (int64_t)page * p.ks_b + ((sk_t0 + j) & pg_tmask) * p.ks_t;
    if constexpr (KTHREAD) return uniform_load4(sp);
    else return make_float4(uniform_load1(sp), 0.f, 0.f, 0.f);
  };
  auto scales_from = [&](const float4 kk, float& sc0, float& sc1) __attribute__((always_inline)) {
    if constexpr (KTHREAD) {
      sc0 = __builtin_fmaf(kk.z, qsc_hi, kk.x * qsc_lo);
      sc1 = __builtin_fmaf(kk.w, qsc_hi, kk.y * qsc_lo);
    } else {
      sc0 = sc1 = qsc * kk.x;
    }
  };
  // sequence end and diagonal: register e of block mt holds key 64 * j + 32 * mt + (e & 3) + 8 * (e >> 2) + 4 * hh
  auto mask_limit = [&](const int j, v16i (&s)[2]) __attribute__((always_inline)) {
    const int lim = min(N_ - 1, lim_l) - (j << 6) - 4 * hh;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) s[mt][e] = (32 * mt + (e & 3) + 8 * (e >> 2) <= lim) ? s[mt][e] : kMaskedI;
#ifdef SAGE_ATTN_DECODE_BODY_WINDOW
    // two-sided, lo <= key <= lim, in a second pass of the same select so that only one limit is live at a time; the lower one
    // where the tile needs it (wave uniform)
    if (j < dw_nlm) {
      const int lo = lim_l - (dw_window - 1) - (j << 6) - 4 * hh;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) s[mt][e] = (32 * mt + (e & 3) + 8 * (e >> 2) >= lo) ? s[mt][e] : kMaskedI;
    }
#endif
  };
  // row max of a tile's logits from the raw integers (the scales are positive)
  auto row_max = [&](const v16i (&s)[2], const float sc0, const float sc1) __attribute__((always_inline)) -> float {
    int mxa = s[0][0], mxb = s[0][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if (e & 2) mxb = max(mxb, s[mt][e]); else mxa = max(mxa, s[mt][e]);
      }
    float mx;
    if constexpr (KTHREAD) mx = max_raw((__int_as_float(mxa) - kBiasF) * sc0, (__int_as_float(mxb) - kBiasF) * sc1);
    else mx = (__int_as_float(max(mxa, mxb)) - kBiasF) * sc0;
    return swap_max(mx);
  };
  // lazy rescale: only when some row's maximum grew by more than the threshold (fp8: p carries the exponent offset 8.807 - 3)
  constexpr float kLazyThr = PV_FP8 ? 3.0f : 6.0f;
  constexpr float kPOff = PV_FP8 ? 8.807f - 3.0f : 0.f;
  float m_thr = m_run + kLazyThr;
  auto maybe_rescale = [&](const float mx) __attribute__((always_inline)) {
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(mx > m_thr) != 0, 0)) {
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      m_thr = m_new + kLazyThr;
      l_run *= alpha;
      if constexpr (MROW) l4 *= alpha;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc_o[dt][e] *= alpha;
    }
  };
  // p = exp2(t - m) and O^T += V^T . P^T of one tile out of V slot `slot`
  auto softmax_pv = [&](const int slot, const v16i (&s)[2], const float sc0, const float sc1) __attribute__((always_inline)) {
    const float c0 = __builtin_fmaf(-kBiasF, sc0, kPOff - m_run), c1 = __builtin_fmaf(-kBiasF, sc1, kPOff - m_run);
    auto prob = [&](const int mt, const int e) __attribute__((always_inline)) -> float {
      const bool g1 = (e & 2) != 0;
      return __builtin_amdgcn_exp2f(__builtin_fmaf(__int_as_float(s[mt][e]), g1 ? sc1 : sc0, g1 ? c1 : c0));
    };
    if constexpr (!PV_FP8) {
      // quarters of 16 keys: the quarter's P pairs (row sums in pair order), then its P.V MFMAs
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int mt = q >> 1, sq = q & 1;
        v8h pf;
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          const v2f pp = {prob(mt, 8 * sq + e), prob(mt, 8 * sq + e + 1)};
          v2h ph;
          if constexpr (V_BF16) ph = __builtin_bit_cast(v2h, __builtin_convertvector(pp, v2bf));
          else ph = __builtin_convertvector(pp, v2h);
          pf[e] = ph[0];
          pf[e + 1] = ph[1];
          if constexpr (!MROW) {
            l_run += pp[0];
            l_run += pp[1];
          }
        }
        if constexpr (MROW) l4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(sel8, pf, l4, 0, 0, 0);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const char* base = v_rd[dt] + (slot * VBYTES + 16 * q * (2 * D));
          const v4s_vs lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_vs*)(base));
          const v4s_vs hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_vs*)(base + 8 * (2 * D)));
          v8h a;
          a.s0123 = __builtin_bit_cast(v4h, lo);
          a.s4567 = __builtin_bit_cast(v4h, hi);
          if constexpr (V_BF16)
            acc_o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, pf), acc_o[dt], 0, 0, 0);
          else
            acc_o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pf, acc_o[dt], 0, 0, 0);
        }
      }
    } else {
      // all 64 keys in one K = 64 MFMA per d tile; P^T bytes in accumulator order 16 * mt + reg
      v8i pb;
      float psum = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        const int mt = w >> 2, e0 = 4 * (w & 3);
        const float p0 = prob(mt, e0), p1 = prob(mt, e0 + 1), p2 = prob(mt, e0 + 2), p3 = prob(mt, e0 + 3);
        psum += p0; psum += p1; psum += p2; psum += p3;
        int pk = 0;
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(p0, p1, pk, false);  // OCP e4m3, RNE
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(p2, p3, pk, true);
        pb[w] = pk;
      }
      l_run += psum;
      if constexpr (PV_FP4) {  // out of the register stage: no LDS read
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc_o[dt] = pv4_mfma(dt, pb, acc_o[dt]);
        return;
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int base = slot * VBYTES + dt * 32 * 64;
        v8i a;
        a.s0123 = *reinterpret_cast<const v4i*>(v_rd8[0] + base);
        a.s4567 = *reinterpret_cast<const v4i*>(v_rd8[1] + base);
        acc_o[dt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, pb, acc_o[dt], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
      }
    }
  };

  // ---- prologue: the pages of the first tiles in one scalar round trip, K(0), K(1) and V(0) in flight beside the Q quantizer
  const int pg0 = page_at(0);
  int pg1 = page_at(1), pg2 = page_at(2);  // the pages of tiles j + 1 and j + 2 (clamped) while iteration j runs
  dma_k(0, 0, pg0);
  if (ntiles > 1) dma_k(1, 1, pg1);
  fetch_v(0, 0, pg0);
  prepare_q();
  qsc_lo = hh ? 0.f : qsc;
  qsc_hi = hh ? qsc : 0.f;
  if (ntiles > 1) dma_wait_keep<NK + NVM>(); else dma_wait_keep<NVM>();  // K(0) has landed

  v16i s_a[2], s_b[2];
  float a0, a1, b0 = 0.f, b1 = 0.f, mx_cur;
  qk(0, s_a);
  scales_from(load_kscales(0, pg0), a0, a1);
  if (SAGE_DECODE_TILE_MASKED(0)) mask_limit(0, s_a);
  mx_cur = row_max(s_a, a0, a1);
  float4 kk_nxt = load_kscales(min(1, last_tile), pg1);

  // Iteration j: S(j) and its row maximum are known.  SLOT = j % 2 at compile time: K(j) and V(j) live in slot SLOT, K(j + 1)
  // and V(j + 1) in the other one.
  auto iter = [&](auto slot_tag, const int j, v16i (&sa)[2], v16i (&sb)[2], float& c0, float& c1, float& n0, float& n1)
      __attribute__((always_inline)) {
    constexpr int SLOT = decltype(slot_tag)::value;
    const bool has_next = j + 1 < ntiles;
    // the copies of this iteration: K(j + 2) over K(j), whose S is done, and V(j + 1) over V(j - 1), whose P.V is done.  Then
    // the counted wait: everything older than this iteration's copies has landed, K(j + 1) and V(j) among it.
    lds_reads_done();
    const int pg3 = page_at(j + 3);
    if constexpr (PV_FP4) {
      // ... PV_FP4: K(j + 2) alone; V(j) was loaded behind the P.V of tile j - 1 and stays in flight until this tile's P.V
      if (j + 2 < ntiles) {
        dma_k(j + 2, SLOT, pg2);
        dma_wait_keep<NK + NVM>();  // K(j + 1) has landed; V(j) and K(j + 2) are younger
      } else {
        dma_wait_all();
      }
    } else if (j + 2 < ntiles) {
      dma_k(j + 2, SLOT, pg2);
      fetch_v(j + 1, SLOT ^ 1, pg1);
      dma_wait_keep<NK + NVM>();
    } else if (has_next) {
      fetch_v(j + 1, SLOT ^ 1, pg1);
      dma_wait_keep<NVM>();
    } else {
      dma_wait_all();
    }
    maybe_rescale(mx_cur);
    if (has_next) {  // S(j + 1): independent of the softmax of tile j, so its MFMAs run beside the exponentials
      scales_from(kk_nxt, n0, n1);
      kk_nxt = load_kscales(min(j + 2, last_tile), pg2);
      qk(SLOT ^ 1, sb);
      if (SAGE_DECODE_TILE_MASKED(j + 1)) mask_limit(j + 1, sb);
    }
    if constexpr (PV_FP4) {  // V(j) has landed: only K(j + 2) is younger
      if (j + 2 < ntiles) dma_wait_keep<NK>();
      v4_landed();
    }
    softmax_pv(SLOT, sa, c0, c1);
    if constexpr (PV_FP4) {  // behind the last MFMA that reads the registers: V(j + 1), out of tile j + 1's page
      if (has_next) fetch_v(j + 1, SLOT ^ 1, pg1);
    }
    if (has_next) mx_cur = row_max(sb, n0, n1);
    pg1 = pg2;
    pg2 = pg3;
  };
  int j = 0;
  for (; j + 1 < ntiles; j += 2) {
    iter(std::integral_constant<int, 0>{}, j, s_a, s_b, a0, a1, b0, b1);
    iter(std::integral_constant<int, 1>{}, j + 1, s_b, s_a, b0, b1, a0, a1);
  }
  if (j < ntiles) iter(std::integral_constant<int, 0>{}, j, s_a, s_b, a0, a1, b0, b1);

  // ---- epilogue: the normalised fp32 partial of the split and its raw base-2 LSE into the workspace slot of (split, b, h, row)
  const float l_tot = MROW ? ((row & 16) ? l4[1] : l4[0]) : swap_sum(l_run);
  const float inv = 1.0f / l_tot;
#ifdef SAGE_ATTN_DECODE_BODY_WINDOW
  // The finish inside the launch (one split): no partial is written.  The lane does what window_merge_row
  // (sage_attn_splitkv_window.hip) does for count == 1 with the values it would have stored -- that function's operations in its
  // order, its library calls, ONE rounding of the output -- so the row has the bits of the two-launch path.
  // Lane (row, hh) holds 4 neighbouring channels per (dt, g4): one 8-byte store each, as a thread of the merge.
  if (dw_fused) {
    if (row >= M_) return;
    const float l0 = m_run + log2f(l_tot) - kPOff;  // the raw base-2 LSE of the split
    const float mx = fmaxf(-INFINITY, l0);
    const bool use = l0 != -INFINITY;               // (a row without a key: o = 0, lse = -inf)
    const float w = exp2f(l0 - mx);
    float sum = 0.f;
    sum = use ? sum + w : sum;
    const float minv = sum > 0.f ? 1.0f / sum : 0.f;
    float v, keep = 1.0f;
    {
#pragma clang fp contract(off)
      v = (sum > 0.f ? mx + log2f(sum) : -INFINITY) / 1.44269504f;
      v += (p.lse ? dw_corr : 0.f) * p.sm_scale;
      if (dw_sinks && sum > 0.f) {
        const float sk = dw_sinks[h * p.q_fold + row % p.q_fold];
        const float top = fmaxf(v, sk);
        const float v2 = top + logf(expf(v - top) + expf(sk - top));
        keep = expf(v - v2);
        v = v2;
      }
    }
    const float kf = dw_sinks ? minv * keep : minv;
    uint16_t* const op = p.o + b * p.osb + h * p.osh + (int64_t)row * p.osn + 4 * hh;
    auto finish = [&](auto bf16_tag) __attribute__((always_inline)) {
      constexpr bool BF16 = decltype(bf16_tag)::value;
      // a * kf rounded ONCE to fp16, as the merge's statement comes out of hipcc there (v_fma_mixlo_f16: product and convert
      // in one instruction).  Here the same statement came out as that instruction for some elements of the unrolled store
      // and as a multiply and a convert -- two roundings, an ulp apart in one element of a few thousand -- for others, so the
      // instruction is named.  bf16 has no such instruction: product, then convert, in both kernels.
      auto rounded = [&](const float a) __attribute__((always_inline)) -> uint32_t {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (!BF16) {
          uint32_t bits;
          asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(bits) : "v"(a), "v"(kf));
          return bits & 0xffffu;
        }
#endif
        return (uint32_t)f32_to_elem_bits<BF16>(a * kf);
      };
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int d0 = 32 * dt + 8 * g4;
          float x[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] = acc_o[dt][4 * g4 + e] * inv;
          if constexpr (PV_FP8 && !PV_FP4) {
            const float4 vs = *reinterpret_cast<const float4*>(p.v_scale + ((int64_t)b * p.Hk + hk) * D + d0 + 4 * hh);
            x[0] *= vs.x; x[1] *= vs.y; x[2] *= vs.z; x[3] *= vs.w;
          }
          float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = use ? acc[e] + x[e] * w : acc[e];
          uint2 w2;
          w2.x = rounded(acc[0]) | (rounded(acc[1]) << 16);
          w2.y = rounded(acc[2]) | (rounded(acc[3]) << 16);
          *reinterpret_cast<uint2*>(op + d0) = w2;
        }
    };
    if (p.out_bf16) finish(std::true_type{}); else finish(std::false_type{});
    if (hh == 0 && p.lse) p.lse[((int64_t)b * p.Hq + h) * M_ + row] = v;
    return;
  }
#endif
  if (row < M_) {
    const int64_t srow = ((((int64_t)split * p.B + b) * p.Hq + h) * M_ + row);
    float* const wp = p.sk_o + srow * D + 4 * hh;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d0 = 32 * dt + 8 * g4;
        float x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = acc_o[dt][4 * g4 + e] * inv;
        if constexpr (PV_FP8 && !PV_FP4) {  // (PV_FP4: the block scales went into the MFMA; p.v_scale holds their bytes)
          const float4 vs = *reinterpret_cast<const float4*>(p.v_scale + ((int64_t)b * p.Hk + hk) * D + d0 + 4 * hh);
          x[0] *= vs.x; x[1] *= vs.y; x[2] *= vs.z; x[3] *= vs.w;
        }
        *reinterpret_cast<float4*>(wp + d0) = make_float4(x[0], x[1], x[2], x[3]);
      }
    if (hh == 0) p.sk_lse[srow] = m_run + log2f(l_tot) - kPOff;
  }
#undef SAGE_DECODE_TILE_MASKED
