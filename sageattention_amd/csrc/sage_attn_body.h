// The body of the attention kernels: included INTO attn_i8_kernel and attn_i8_blocksparse_kernel (sage_attn.hip),
// attn_i8_blocksparse_pvskip_kernel (sage_attn_pvskip.hip), attn_i8_kvlen_kernel (sage_attn_kvlen.hip),
// attn_i8_blocksparse_kvlen_kernel (sage_attn_sparse_kvlen.hip) and attn_i8_blocksparse_pvskip_kvlen_kernel
// (sage_attn_sparse_kvlen_pvskip.hip), attn_i8_splitkv_kernel (sage_attn_splitkv.hip) and attn_i8_splitkv_causal_kernel
// (sage_attn_splitkv_causal.hip), not a header in the usual sense.
// Expects in scope: the kernel parameter block `p` and the compile-time constants D, NWAVES, CAUSAL, KTHREAD, V_BF16, PV_FP8,
// HAS_MASK, SPARSE, PVSKIP, KVLEN, SPLITKV, PAGED
// (PAGED, with SPLITKV only: attn_i8_splitkv_paged_kernel / attn_i8_splitkv_causal_paged_kernel, sage_attn_splitkv_paged.hip /
// sage_attn_splitkv_causal_paged.hip -- K, V and the K scales are pools of pages and tile j of the batch comes from the page
// its block-table row names, through a descriptor of its own; every other kernel defines PAGED = false)
// (see those files for what they select; KVLEN: attn_i8_kvlen_kernel, sage_attn_kvlen.hip; SPARSE && KVLEN: the tile lists
// clipped at the batch's length, sage_attn_sparse_kvlen.hip; SPLITKV: one workgroup per (b, h, q-block, split) walks the
// split's range of key tiles and stores an fp32 partial result, sage_attn_splitkv.hip; CAUSAL && SPLITKV: the diagonal is
// aligned to the END of the batch's keys and counts tokens of p.q_fold query rows, sage_attn_splitkv_causal.hip).
#ifndef SAGE_ATTN_BODY_OF_KERNEL
#error "sage_attn_body.h is the body of the attention kernels (sage_attn*.hip): included nowhere else"
#endif
  static_assert(!(PV_FP8 && V_BF16), "fp8 V has no bf16 flavour");
  static_assert(!HAS_MASK || (!CAUSAL && !PV_FP8), "attn_mask: non-causal 16-bit-PV operator");
  static_assert(!SPARSE || (NWAVES == 4 && !CAUSAL && !HAS_MASK), "block-sparse: 4 waves = one block row of the map, non-causal");
  static_assert(!PVSKIP || SPARSE, "the P.V skip exists in the block-sparse form only");
  static_assert(!KVLEN || !HAS_MASK, "per-batch key lengths: the dense or the block-sparse kernel, without attn_mask");
  static_assert(!SPLITKV || (!HAS_MASK && !SPARSE && !KVLEN && NWAVES == 4),
                "split-KV: 4 waves, no attn_mask, no block map (its optional lengths are its own: p.kv_lens may be null)");
  static_assert(!PAGED || SPLITKV, "block tables: the split-KV kernels only");
  constexpr int T = NWAVES * 64;
  constexpr int QB = NWAVES * 32;
  constexpr int KS = D / 32;          // k-steps of the int8 QK^T MFMA
  constexpr int DT = D / 32;          // 32-wide d tiles of O^T
  constexpr int KBYTES = 64 * D;      // one K tile (int8)
  constexpr int VBYTES = PV_FP8 ? 64 * D : 64 * D * 2;  // one V tile: fp16 [64][D] or e4m3 [D][64]
  constexpr int KCH = D / 16;         // 16-B chunks per K row
  constexpr int VCH = PV_FP8 ? 4 : D / 8;       // 16-B chunks per V tile row (fp8: a V^T row holds 64 tokens)
  constexpr int VROWS = PV_FP8 ? D : 64;        // rows of the V tile image
  constexpr int KC = (64 * KCH + T - 1) / T;    // chunks per thread
  constexpr int VC = (VROWS * VCH + T - 1) / T;
  static_assert(PV_FP8 || (64 * VCH) % T == 0, "V tile must divide over the workgroup");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const k_lds = smem;
  // K/V tile ring in LDS.  FP16 PV: two slots each (K fetched two tiles ahead, V one; every tile copy has ONE iteration to
  // land and is drained with vmcnt(0) in front of the barrier that publishes it).  FP8 PV: four slots each, K fetched four
  // tiles ahead and V three, and the per-tile wait leaves the copies of the last two iterations in flight (counted vmcnt):
  // a copy has three iterations to land, which takes the L2 round trip off the critical path (measured bound of that
  // latency on the FP8 loop, same-tile ablation: +4.8 %; tiles are half as big, so the ring costs 64 KiB at head_dim 128).
  // (counted waits need every wave to issue the same number of copies per tile: not so when a tile has fewer 16-B
  // chunks than the workgroup has threads -- head_dim 64 with 8 waves, a tuning-only geometry, keeps two slots)
  constexpr int RING = attn_ring_slots(D, NWAVES, PV_FP8);
  char* const v_lds = smem + RING * KBYTES;

  // ---- block -> (b, h, q block), XCD aware: consecutive logical ids (same head) share an L2
  const int nwg = gridDim.x;
  int lid;
  {
    const int orig = blockIdx.x, xcd = orig & 7, qq = nwg >> 3, rr = nwg & 7;
    lid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (orig >> 3);
  }
  // split-KV: the splits of one (b, h, q-block) are neighbours -- they read the same Q rows -- and the id above them is that of
  // the other kernels
  int split = 0;
  (void)split;
  if constexpr (SPLITKV) {
    split = lid % p.num_splits;
    lid /= p.num_splits;
  }
  int qb = lid % p.nqb;
  const int bh = lid / p.nqb;
  // (b, h) of the id: heads within a batch -- except with per-batch key lengths, where the batches alternate within a head.
  // An XCD runs one contiguous range of logical ids; batch-major, an XCD would hold whole batches, and the one with the
  // longest batch would finish last whatever the others save (lengths 8192 / 6144 / 4096 / 2048: 0.96x the dense time)
  const int h = (KVLEN || SPLITKV) ? bh / p.B : bh % p.Hq, b = (KVLEN || SPLITKV) ? bh % p.B : bh / p.Hq;
  // Causal: heaviest q-blocks of a head first (load balance at the end of the grid).  An XCD holds fewer workgroups than
  // a long head has q-blocks, so a head runs in two generations and the second starts again at key 0 (C4 reads 2.06x its
  // K/V + Q bytes from the HBM side, 1.72x with 8-wave workgroups: profiles/r03_ab/fetch_by_geometry.md; at 0.35 TB/s).
  // Lightest first measured 1-2 % slower on every causal shape, with more HBM-side reads.
  if constexpr (CAUSAL) qb = p.nqb - 1 - qb;
  const int hk = h / (p.Hq / p.Hk);
  // the list row (and the skip counters) of the workgroup are those of (b, h): the id itself, but for the batch interleave above
  const int bh_row = (SPARSE && KVLEN) ? b * p.Hq + h : bh;
  int M_ = p.M, N_ = p.N;
  int64_t q_boff = b * p.qsb, k_boff = b * p.ksb, v_boff = b * p.vsb, o_boff = b * p.osb;
  if (p.cu_q) {  // packed sequences: wave-uniform, before any barrier
    const int q_lo = p.cu_q[b], k_lo = p.cu_k[b];
    M_ = p.cu_q[b + 1] - q_lo;
    N_ = p.cu_k[b + 1] - k_lo;
    if (qb * QB >= M_) return;
    q_boff = (int64_t)q_lo * p.qsn; o_boff = (int64_t)q_lo * p.osn;
    k_boff = (int64_t)k_lo * p.ksn; v_boff = (int64_t)k_lo * p.vsn;
    if (N_ <= 0) {  // a sequence with queries but no keys: the reference stores zeros (acc = 0, l_i = 1;
                    // attn_qk_int8_block_varlen.py:109-121), it does not leave the rows unwritten
      const int rows = min(QB, M_ - qb * QB);
      uint16_t* ob = p.o + o_boff + h * p.osh + (int64_t)(qb * QB) * p.osn;
      for (int i = threadIdx.x; i < rows * (D / 4); i += T)
        *reinterpret_cast<uint2*>(ob + (int64_t)(i / (D / 4)) * p.osn + (i % (D / 4)) * 4) = make_uint2(0u, 0u);
      return;
    }
  }
  if constexpr (KVLEN) {  // per-batch key lengths: wave-uniform, before any barrier.  Everything below follows N_ -- the tile
                          // range, the tail mask and the K / V descriptors, which end with row N_ - 1 (rows beyond read as zeros)
    N_ = min(max(uniform_load_i32(p.kv_lens + b), 0), p.N);
    // a batch without keys: nothing to do here.  Its rows are DEFINED, o = 0 as for a packed sequence without keys above and
    // lse = -inf: attn_kvlen_empty_kernel writes them.  (Written here, the stores cost the head_dim-64 variants the registers
    // that keep them at three waves per SIMD, and FP8 PV with per-thread scales spilled -- as in the block-sparse form below.)
    if (N_ <= 0) return;
  }
  // split-KV: split s of a batch with ntk_b = ceil(len_b / 64) key tiles owns the tiles [s * tps_b, min((s + 1) * tps_b, ntk_b)),
  // tps_b = ceil(ntk_b / S) (the rule: include/sageattn_hip.h, sage_attn_fusedq_pv_*_splitkv).  The workgroup is the dense
  // kernel on that range: sk_t0 moves the K / V slice and the K scales to the range's first tile (below) and N_ becomes the keys
  // from there to the range's end -- a multiple of 64 for every split but the one that holds the batch's last tile, whose tail
  // mask and descriptors then end at len_b.  Tile indices, ring slots and the ragged-tail logic are those of the dense kernel
  // on the moved operands.  Wave-uniform, before any barrier; a workgroup whose range is empty stores nothing.
  int sk_t0 = 0;
  (void)sk_t0;
  // causal split-KV (the rule: include/sageattn_hip.h, sage_attn_fusedq_pv_*_splitkv_causal): row r is token t = r / g,
  // g = p.q_fold, and attends the keys j <= t + off_b, off_b = len_b - M / g: the M / g tokens are the LAST positions of the
  // batch's len_b keys.  sk_off is off_b in the coordinates of the moved operands, off_b - 64 * sk_t0 = (keys from the split's
  // first one to len_b) - M / g: the first term is positive for a split that runs, so the difference cannot overflow.
  int sk_off = 0;
  (void)sk_off;
  if constexpr (SPLITKV) {
    int len_b = p.N;
    if (p.kv_lens) len_b = min(max(uniform_load_i32(p.kv_lens + b), 0), p.N);
    const int ntk_b = (len_b + 63) >> 6, tps_b = (ntk_b + p.num_splits - 1) / p.num_splits;
    sk_t0 = split * tps_b;
    const int t1 = min(sk_t0 + tps_b, ntk_b);
    if (sk_t0 >= t1) return;
    N_ = min(len_b, t1 << 6) - (sk_t0 << 6);
    if constexpr (CAUSAL) sk_off = (len_b - (sk_t0 << 6)) - M_ / p.q_fold;
  }
  // block-sparse: the list row of this (b, h, q-block) = its count, then the ascending tile indices, padded with the last
  // valid one for kBlockListPad entries so that every read-ahead below is blind.  The first entries are requested together
  // with the count: one scalar round trip in front of the first tile copies.
  const int* bsl = nullptr;
  int bs_count = 0, bs_first[5] = {0, 0, 0, 0, 0};
  float pv_thr = 0.f;  // PVSKIP: the head's threshold (sage_attn_*_blocksparse_pvskip), in base-2 logit units below
  (void)pv_thr;
  if constexpr (SPARSE) {
    bsl = p.bs_lists + ((int64_t)bh_row * p.nqb + qb) * p.bs_row;
    bs_count = uniform_load_i32(bsl);
    if constexpr (PVSKIP) pv_thr = uniform_load1(p.pv_thresh + h);
    ++bsl;
#pragma unroll
    for (int i = 0; i < 5; ++i) bs_first[i] = uniform_load_i32(bsl + i);
    if constexpr (KVLEN) {
      // The list is the caller's, made for N keys and read-only: of a batch that ends earlier only the entries < ntk_b =
      // ceil(len_b / 64) count, and the list ascends, so they are a prefix.  Its length by a ballot count over the row: every
      // wave counts for itself (wave uniform, before any barrier), lane l looks at entries l, l + 64, l + 128, l + 192 of a
      // 256-entry chunk, all four loads in flight together, and the counts are scalar popcounts -- nothing of it lives on into
      // the loop.  A batch of full length (ntk_b = ceil(N / 64)) does not look.  The entries behind the prefix name real tiles
      // beyond the length: the blind read-ahead below may copy them -- K comes back as zeros, the descriptor ends with row
      // len_b - 1 -- but their ring slots belong to list positions >= the clipped count, which no wave computes.
      const int ntk_b = (N_ + 63) >> 6;
      if (ntk_b < ((p.N + 63) >> 6)) {
        const int ln = threadIdx.x & 63;
        int cnt = 0;
        for (int base = 0; base < bs_count; base += 256) {
          int e[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) e[u] = bsl[min(base + 64 * u + ln, bs_count - 1)];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(base + 64 * u + ln < bs_count && e[u] < ntk_b));
        }
        bs_count = cnt;
      }
    }
    // an empty q-block: nothing to do here, before any barrier (wave uniform).  Its rows are DEFINED, o = 0 and lse = -inf:
    // attn_blocksparse_empty_kernel writes them.  (Written here, the stores cost the head_dim-64 variants the registers
    // that keep them at three waves per SIMD -- FP8 PV with per-thread scales spilled its bias tuple.)
    if (bs_count <= 0) return;
  }
  // key tile at list position `pos` (dense: the position itself)
  auto tile_at = [&](const int pos) __attribute__((always_inline)) -> int {
    if constexpr (SPARSE) return uniform_load_i32(bsl + pos); else return pos;
  };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int q0 = qb * QB + wave * 32;
  const int row = q0 + r;
  const int rowc = min(row, M_ - 1);
  // PVSKIP: the lanes whose rows take part in the skip decision (rows >= M do not: the padded rows of a ragged q-block
  // would veto every skip), as a 64-bit lane mask in scalar registers; the skipped tiles of this wave, counted in one
  uint64_t pv_rows = 0;
  int n_skipped = 0;
  (void)pv_rows; (void)n_skipped;
  if constexpr (PVSKIP) {
    const int nvalid = min(32, max(0, M_ - q0));
    const uint64_t half = nvalid >= 32 ? 0xffffffffull : ((1ull << nvalid) - 1ull);
    pv_rows = half | (half << 32);
    // a threshold that is not a positive finite number (<= 0, +inf, NaN) never skips
    pv_thr = (pv_thr > 0.f && pv_thr < __builtin_huge_valf()) ? pv_thr * 1.44269504f : __builtin_huge_valf();
  }
  // the lane's row / key-half as the masked tiles and the epilogue see them: re-derived from the lane id after the fast loop
  // (below), so that neither they nor the output addresses built from them occupy registers while it runs
  int row_l = row, hh_l = hh;
  // causal split-KV: the last key (of the moved operands) the lane's row may attend, token + sk_off, what `row_l` is to the
  // top-left diagonal of the dense kernel.  Every negative limit means "no key of this split" and is held at -1, so that the
  // tile offsets mask_limit subtracts from it cannot wrap.  Rows >= M are never stored.  One divide per lane here, for tile 0,
  // and one more behind the fast loop, where row_l is re-derived: kept in a register through the loop instead, the limit
  // costs the head_dim-64 FP8 variant with per-thread scales its third wave per SIMD (168 registers and 84 bytes of scratch).
  int lim_l = 0, sk_tok0 = 0, sk_tok1 = 0;  // ... and the tokens of the wave's first row and of its last row < M
  (void)lim_l; (void)sk_tok0; (void)sk_tok1;
  if constexpr (CAUSAL && SPLITKV) {
    lim_l = max(row / p.q_fold + sk_off, -1);
    sk_tok0 = q0 / p.q_fold;
    sk_tok1 = min(q0 + 31, M_ - 1) / p.q_fold;
  }

  // ---- Q^T fragments (B operand), resident for the whole kernel, and the per-row q scale
  // (a lambda: it runs AFTER the first K/V tile copies have been issued, below -- nothing in it depends on them, and with
  //  one workgroup per CU nobody else hides the latency of its loads; the copies and the Q loads then fly together)
  v4i qf[KS];
  float qsc;
  auto prepare_q = [&]() __attribute__((always_inline)) {
  if (p.q_f16 == nullptr) {
    const int8_t* qp = p.q + q_boff + h * p.qsh + (int64_t)rowc * p.qsn + 16 * hh;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const v4i*>(qp + 32 * ks);
    int qi;  // …sm80.cu:103-117 index maps, evaluated once per lane
    if (p.qgran == SAGE_GRAN_PER_BLOCK) qi = rowc / p.blkq;
    else if (p.qgran == SAGE_GRAN_PER_WARP) qi = rowc / p.warpq;
    else qi = (rowc / p.warpq) * 8 + (rowc & 7);
    qsc = p.q_scale[((int64_t)b * p.Hq + h) * p.gq + qi] * p.logit_mult;
  } else {
    // Fused Q quantizer (replaces one launch of K1 and the q8 round trip through HBM).  Lane (r, hh) owns the 16-column
    // chunks [32*ks + 16*hh, +16) of its row: exactly the bytes of its B fragments.  Same arithmetic as K1, so q8 and
    // the scales are bit-identical to the stand-alone quantizer; rows >= M are zeros, as there.
    const bool valid = row < M_;
    const uint16_t* qp = p.q_f16 + q_boff + h * p.qsh + (int64_t)rowc * p.qsn + 16 * hh;
    uint4 raw[KS][2];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      raw[ks][0] = *reinterpret_cast<const uint4*>(qp + 32 * ks);
      raw[ks][1] = *reinterpret_cast<const uint4*>(qp + 32 * ks + 8);
    }
    // (the LSE correction q . k_mean is only computed when the caller asked for the LSE)
    const uint16_t* kmp = (p.km && p.lse) ? p.km + ((int64_t)b * p.Hk + hk) * D + 16 * hh : nullptr;
    // (split-KV: the correction of a row is computed and parked once, by the workgroup of split 0 -- the merge consumes it)
    if constexpr (SPLITKV) {
      if (split != 0) kmp = nullptr;
    }
    // Everything below is instantiated per element type (ONE uniform branch here instead of one per 8-element chunk) and
    // the numerics flavour is the kernel's KTHREAD (per-thread Q scales <=> the Triton quantizer's numerics, run_attn): with
    // both as run-time flags inside the unrolled loops hipcc emitted two scalar branches per ELEMENT -- ~500 scalar
    // instructions and as many taken branches per wave, a third of a short sequence's fixed cost.
    auto fused_q = [&](auto bf16_tag) __attribute__((always_inline)) {
    constexpr bool QBF = decltype(bf16_tag)::value;
    constexpr bool triton = KTHREAD;
    if (!valid) {  // rows >= M are zeros (as in K1): zeroed once here, 4 selects per chunk instead of 8 per pass
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
    // LSE correction q . k_mean of the row: parked in the caller's LSE slot of this row until the epilogue (a register that
    // lives through the whole tile loop costs the head_dim-64 FP8 variants their third wave per SIMD)
    const float lse_corr = swap_sum(dot);
    // (the two forms are spelled out under `if constexpr`, as is the km pointer above: with `(!SPLITKV || split == 0)` as a term
    //  of the one condition, the FP8 head_dim-64 block-sparse kernels came out with another instruction stream)
    if constexpr (SPLITKV) {
      if (split == 0 && p.lse && hh == 0 && valid) p.lse[((int64_t)b * p.Hq + h) * M_ + row] = lse_corr;
    } else {
      if (p.lse && hh == 0 && valid) p.lse[((int64_t)b * p.Hq + h) * M_ + row] = lse_corr;
    }
    if constexpr (triton) {  // rows with equal r % 8 inside the 32-row block (quant_per_thread.py:27-36)
      amax = fmaxf(amax, __shfl_xor(amax, 8));
      amax = fmaxf(amax, __shfl_xor(amax, 16));
    } else {       // per warp: warpq rows (16 or 32) share a scale (fused.cu:746-750)
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
      if (p.warpq == 32) amax = fmaxf(amax, __shfl_xor(amax, 16));
    }
    const float a_c = fmaxf(amax, 0.0000001f);
    const float sc = triton ? amax / 127.f + 0.0000001f : a_c / 127.f;
    const float inv = 127.f / a_c;
    const float rcp_sc = 1.0f / sc;
    // Triton numerics need x/sc correctly rounded before the half-away rounding; as in K1 the reciprocal product is
    // used unless some value of the wave's 8-column chunk lands within 2^-14 of a rounding boundary (then the exact
    // division decides, for that chunk: ~6 % of the chunks; deciding once for the wave's whole 32 x D block sent
    // 40 % of the waves through the slow form)
    const bool rcp_bad = !(fabsf(rcp_sc) < 3.0e38f);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      uint32_t w[4];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float f[8];
        unpack8<QBF>(raw[ks][c], f);
        int qv[8];
        // (no clamp on the two fast forms: |f| <= amax, so |f * r| <= 127 (1 + 3 ulp) and rint() of it is at most 127; as K1)
        if constexpr (triton) {
          bool near = false;
#pragma unroll
          for (int e = 0; e < 8; ++e) qv[e] = round_half_away_fast(f[e] * rcp_sc, near);
          if (__builtin_amdgcn_ballot_w64(near || rcp_bad) != 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              float y = f[e] / sc;  // IEEE division (quant_per_thread.py:41)
              y = y + (y >= 0.f ? 0.5f : -0.5f);
              qv[e] = min(max((int)y, -128), 127);
            }
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) qv[e] = (int)rintf(f[e] * inv);  // cvt.rni (fused.cu:176-181)
        }
        w[2 * c] = pack_i8x4(qv[0], qv[1], qv[2], qv[3]);
        w[2 * c + 1] = pack_i8x4(qv[4], qv[5], qv[6], qv[7]);
      }
      qf[ks][0] = (int)w[0]; qf[ks][1] = (int)w[1]; qf[ks][2] = (int)w[2]; qf[ks][3] = (int)w[3];
    }
    qsc = sc * p.logit_mult;
    };
    if (p.q_bf16) fused_q(std::true_type{}); else fused_q(std::false_type{});
  }
  };
  const float* ksp = p.k_scale + b * p.ks_b + hk * p.ks_h;
  if constexpr (SPLITKV) ksp += (int64_t)sk_t0 * p.ks_t;

  // ---- tile range
  // (causal split-KV: up to the key bound of the q-block's last row < M.  A workgroup none of whose rows has a key in this
  //  split stores nothing -- the merge derives the same count of splits for the q-block and reads no slot beyond it.  Wave
  //  uniform, before any barrier.)
  int sk_end = 0;
  (void)sk_end;
  if constexpr (CAUSAL && SPLITKV) {
    sk_end = min((qb + 1) * QB - 1, M_ - 1) / p.q_fold + sk_off + 1;
    if (sk_end <= 0) return;
  }
  const int kv_end = CAUSAL ? min(N_, SPLITKV ? sk_end : (qb + 1) * QB) : N_;
  const int ntiles = SPARSE ? bs_count : (kv_end + 63) >> 6;  // block-sparse: list positions
  // (causal split-KV: the tiles up to the bound of the wave's last row, at least one -- a wave whose rows all end before this
  //  split's range computes tile 0, masks all of it and then stages like any causal wave that is done)
  const int wave_tiles = CAUSAL ? min(ntiles, SPLITKV ? max(1, (min(N_, max(sk_tok1 + sk_off, -1) + 1) + 63) >> 6)
                                                      : ((q0 + 31) >> 6) + 1)
                                : ntiles;

  // ---- staging (global -> LDS by LDS-DMA).  Buffer addressing: the descriptor holds the (b, h_kv) slice, the
  //      per-thread byte offset is constant for the whole kernel and the tile advance is a scalar offset, so a
  //      tile costs no address VALU; rows >= N fall outside num_records and read as ZERO (V rows beyond the
  //      sequence must be zero: 0 * garbage could be NaN; K rows beyond it are masked in the softmax).
  const int8_t* kg = p.k + k_boff + hk * p.ksh;
  const uint8_t* vg = p.v + (v_boff + hk * p.vsh) * (PV_FP8 ? 1 : 2);
  const int k_tile_stride = p.k_tile_bytes;  // bytes per 64 keys (dense: 64 rows)
  const int v_tile_stride = p.v_tile_bytes;
  if constexpr (SPLITKV) {  // the slice starts with the split's first tile
    kg += (int64_t)sk_t0 * k_tile_stride;
    vg += (int64_t)sk_t0 * v_tile_stride;
  }
  // last valid byte + 1 of the (b, h_kv) slice: row N-1 = row (N-1)%64 of tile (N-1)/64 (dense layouts: (N-1)*stride_n)
  const int last_t = (N_ - 1) >> 6, last_r = (N_ - 1) & 63;
  const unsigned k_bytes = (unsigned)((int64_t)last_t * k_tile_stride + (int64_t)last_r * p.ksn + D);
  const unsigned v_bytes = PV_FP8 ? (unsigned)((int64_t)last_t * v_tile_stride + (int64_t)(D - 1) * p.vsn + 64)
                                  : (unsigned)((int64_t)last_t * v_tile_stride + ((int64_t)last_r * p.vsn + D) * 2);
  const v4i k_rsrc = make_rsrc(kg, k_bytes), v_rsrc_dma = make_rsrc(vg, v_bytes);
  // LDS-DMA (buffer_load ... lds): a wave instruction writes 64 x 16 B = 1 KiB of LDS LINEARLY (wave-uniform
  // base + 16*lane), so the bank swizzle of the tile image is applied to the per-lane SOURCE offset instead:
  // LDS chunk position c of a tile holds global chunk (row(c), pos(c) ^ swizzle(row)).  No VGPR staging, no
  // ds_write, and the copy has a whole iteration to land (it is drained by the vmcnt(0) of the next barrier).
  // bf16 V is staged like fp16 V (16-bit elements; the transposing LDS read does not care) and multiplied as bf16.
  int k_voff[KC], v_voff[VC];
#pragma unroll
  for (int i = 0; i < KC; ++i) {
    const int c = tid + i * T, kr = c / KCH, pos = c % KCH;
    k_voff[i] = kr * (int)p.ksn + ((pos ^ k_swz<D>(kr)) << 4);
  }
#pragma unroll
  for (int i = 0; i < VC; ++i) {
    const int c = tid + i * T, vr = c / VCH, pos = c % VCH;
    if constexpr (PV_FP8) {
      v_voff[i] = vr * (int)p.vsn + ((pos ^ ((vr >> 2) & 3)) << 4);  // V^T row vr (= channel), 16-B chunk swizzle
    } else {
      const int cc = (((pos >> 2) ^ v_win_swz<D>(vr)) << 2) | (pos & 3);
      v_voff[i] = (vr * (int)p.vsn + cc * 8) * 2;
    }
  }
  // PAGED (the rule: include/sageattn_hip_paged.h).  Tile j of the moved operands is logical tile sk_t0 + j of the batch: tile
  // (sk_t0 + j) % tpp of the page that entry (sk_t0 + j) / tpp of the batch's table row names, tpp = page_size / 64 a power of
  // two.  A page may lie anywhere in a pool of any size, so the tile gets a descriptor of its OWN: words 0-1 are the 64-bit
  // address pool + page * page stride + hk * head stride + tile * tile bytes, formed on the scalar unit, word 2 the bytes of
  // the tile -- of the batch's last tile those up to row len_b - 1, so that the rows behind it (NaN in a recycled page) reach
  // the LDS as zeros exactly as they do through k_bytes / v_bytes above -- and the scalar offset is 0.  Only a tile's own
  // bytes go through a 32-bit offset.  The copies use lds_dma16_fresh: the descriptor is computed in front of every copy, and
  // its wait states stand inside that asm string (sage_attn_common.h).  The page ids come through the scalar cache, requested
  // an iteration ahead like the block-sparse lists (bw1 .. bw4 below hold pages here), with the table index clamped to the
  // one of the range's last tile: no entry at or beyond ceil(len_b / page_size) is read.
  const int8_t* pg_k = nullptr;
  const uint8_t* pg_v = nullptr;
  const float* pg_ks = nullptr;
  const int* pg_row = nullptr;
  int pg_tmask = 0;
  unsigned pg_kfull = 0, pg_klast = 0, pg_vfull = 0, pg_vlast = 0;
  (void)pg_k; (void)pg_v; (void)pg_ks; (void)pg_row; (void)pg_tmask; (void)pg_kfull; (void)pg_klast; (void)pg_vfull; (void)pg_vlast;
  if constexpr (PAGED) {
    pg_k = p.k + hk * p.ksh;
    pg_v = p.v + hk * p.vsh * (PV_FP8 ? 1 : 2);
    pg_ks = p.k_scale + hk * p.ks_h;
    pg_row = p.block_table + (int64_t)b * p.bt_stride;
    pg_tmask = (1 << p.bt_shift) - 1;
    pg_kfull = (unsigned)(63 * (int)p.ksn + D);
    pg_klast = (unsigned)(last_r * (int)p.ksn + D);
    pg_vfull = PV_FP8 ? (unsigned)((D - 1) * (int)p.vsn + 64) : (unsigned)((63 * (int)p.vsn + D) * 2);
    pg_vlast = PV_FP8 ? pg_vfull : (unsigned)((last_r * (int)p.vsn + D) * 2);
  }
  // K(j) -> K buffer `buf` (PAGED: out of page `page`)
  auto dma_k = [&](const int j, const int buf, const int page = 0) __attribute__((always_inline)) {
    if constexpr (PAGED) {
      const uint64_t base = reinterpret_cast<uint64_t>(pg_k) + (uint64_t)((int64_t)page * p.ksb) +
                            (uint64_t)(((sk_t0 + j) & pg_tmask) * k_tile_stride);
      const v4i rs = make_rsrc_uniform(base, j == last_t ? pg_klast : pg_kfull);
#pragma unroll
      for (int i = 0; i < KC; ++i)
        if (KC * T == 64 * KCH || wave * 64 + i * T < 64 * KCH)
          lds_dma16_fresh(rs, (unsigned)(buf * KBYTES + (wave * 64 + i * T) * 16), k_voff[i], 0);
    } else {
#pragma unroll
    for (int i = 0; i < KC; ++i)
      if (KC * T == 64 * KCH || wave * 64 + i * T < 64 * KCH)
        lds_dma16(k_rsrc, (unsigned)(buf * KBYTES + (wave * 64 + i * T) * 16), k_voff[i], j * k_tile_stride);
    }
  };
  // V(j) -> V buffer `buf` (PAGED: out of page `page`)
  auto load_v = [&](const int j, const int buf, const int page = 0) __attribute__((always_inline)) {
    if constexpr (PAGED) {
      const uint64_t base = reinterpret_cast<uint64_t>(pg_v) + (uint64_t)((int64_t)page * p.vsb * (PV_FP8 ? 1 : 2)) +
                            (uint64_t)(((sk_t0 + j) & pg_tmask) * v_tile_stride);
      const v4i rs = make_rsrc_uniform(base, j == last_t ? pg_vlast : pg_vfull);
#pragma unroll
      for (int i = 0; i < VC; ++i) {
        if (!(VC * T == VROWS * VCH || wave * 64 + i * T < VROWS * VCH)) continue;
        lds_dma16_fresh(rs, (unsigned)(RING * KBYTES + buf * VBYTES + (wave * 64 + i * T) * 16), v_voff[i], 0);
      }
    } else {
#pragma unroll
    for (int i = 0; i < VC; ++i) {
      if (!(VC * T == VROWS * VCH || wave * 64 + i * T < VROWS * VCH)) continue;
      lds_dma16(v_rsrc_dma, (unsigned)(RING * KBYTES + buf * VBYTES + (wave * 64 + i * T) * 16), v_voff[i], j * v_tile_stride);
    }
    }
  };
  // ---- lane-constant LDS read offsets
  // (pointers that already include the K / V region base: the fast loops and the generic body then share ONE register per
  // offset; with integer offsets hipcc kept `base + offset` and `offset` as two live values)
  const char* k_rd[KS];  // K A-fragment: row r (+32*mt via immediate), chunk 2*ks+hh
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) k_rd[ks] = k_lds + (r * D + (((2 * ks + hh) ^ k_swz<D>(r)) << 4));
  const char* v_rd8[2];  // fp8: V^T row r (+32*dt immediate), 16-B chunks 2*hh and 2*hh+1
#pragma unroll
  for (int c = 0; c < 2; ++c) v_rd8[c] = v_lds + (r * 64 + (((2 * hh + c) ^ ((r >> 2) & 3)) << 4));
  const char* v_rd[DT];  // fp16: V^T fragment via tr-read: row 4*hh + q4 (+32*mt+16*s(+8) immediate), window dt
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
  // per-lane partial row sum of the UNROUNDED p in fp32 on the VALU (the lane's 32 of the row's 64 keys per tile;
  // the two lane halves are added once in the epilogue), as the reference's Triton kernels and its fp8 CUDA kernel
  // (attn_qk_int8_per_block.py:55-60; ComputeUnit::kCudaCore, sm89_*.cu:148).
  float l_run = 0.f;
  // FP16 PV at head_dim 64: the row sum runs on the matrix pipe instead -- one v_mfma_f32_16x16x32_f16 per 16-key quarter.
  // B = the quarter's 8 packed fp16 p of the lane (MFMA column l%16, k group l/16: lanes l and l+32 are the two halves of
  // query l%16, lanes l+16 and l+48 those of query l%16+16); A[i][k] = 1 iff (k/8) % 2 == i % 2, so the even result rows hold
  // the full row sum of query l%16 and the odd ones that of query l%16+16: elements 0 / 1 of every lane's fp32 accumulator
  // (C is elementwise, so the running sums stay private to the lane and are rescaled by its own alpha).  4 MFMAs of 16 cycles
  // per tile replace 32 v_add_f32 (128 cycles of the vector issue port) and the final lane-half exchange.  It sums the
  // ROUNDED P -- exactly what the reference's fp16 CUDA kernel does (ComputeUnit::kTensorCore: mma::rowsum_f16f16f32 on the
  // packed half P, attn_utils.cuh:528-548, qk_int_sv_f16_cuda_sm80.cu:318-320,814), where its Triton twin sums the fp32 p.
  // At head_dim 64 the loop is bound by vector issue and the matrix pipe is a third busy: steady state C2 +2.7 %, C2-causal
  // +3.1 %, (4,32,8192,64) +3.0 % against the VALU sums, and the unrounded p are dead after the convert (153-156 registers
  // instead of 162-168).  At head_dim 128 every gap already holds a P.V MFMA: +0.2 ... +0.8 % -- not worth giving up the
  // exact fp32 sums there.
  // (bf16 PV keeps the VALU sums of the unrounded p: a sum of bf16-rounded P would cost the LSE three more bits)
  constexpr bool MROW = !PV_FP8 && !V_BF16 && D == 64;
  v4f l4 = {0.f, 0.f, 0.f, 0.f};
  v8h sel8;
  {
    const _Float16 one = (((lane >> 4) & 1) == (lane & 1)) ? (_Float16)1.0f : (_Float16)0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) sel8[e] = one;
    if constexpr (MROW) asm volatile("" : "+v"(sel8));  // resident: as a known value it is re-materialised per use
  }
  auto rowsum8 = [&](const v8h ph) __attribute__((always_inline)) {
    l4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(sel8, ph, l4, 0, 0, 0);
  };
  // The int32 accumulator of S^T starts at the BIT PATTERN of 1.5*2^23: for |S| < 2^22 (|S| <= 128*127^2) the
  // accumulated integer, reinterpreted as fp32, IS the float 12582912 + S exactly, so the logit needs no
  // v_cvt_f32_i32: t - m = fma(as_float(acc), scale, -(12582912*scale + m)).
  constexpr int kBiasI = 0x4B400000;
  constexpr float kBiasF = 12582912.0f;
  // A masked score is the bit pattern of -inf: as an INTEGER it is below every real score (they are ~0x4B400000), so the
  // integer row max ignores it; as a FLOAT it makes fma(-inf, scale, c) = -inf for any positive scale and exp2 returns
  // exactly 0 -- no per-element zeroing of p, no mask bits to carry from the S tile to the P tile.
  constexpr int kMaskedI = (int)0xFF800000u;
  v16i bias;
#pragma unroll
  for (int e = 0; e < 16; ++e) bias[e] = kBiasI;
  // keep the 16 bias registers resident: as a known constant the compiler re-materialises them with 8 v_mov_b64 per
  // tile (or, in the in-place form below, 16 moves per S chain), and the kernel is bound by the vector issue port (every
  // VALU instruction costs 4 cycles of it).  Not in the attn_mask instantiation, which has no registers to spare.  Every
  // dispatched head_dim-64 variant fits WITH the pin (153-168 registers, no scratch; the build fails otherwise): C2-causal
  // +3.1 ... +4.9 %, C2-fp8 +3.9 %, (4,32,8192,64)-fp8 +4.0 %.
  constexpr bool BIAS_RESIDENT = !HAS_MASK;
  if constexpr (BIAS_RESIDENT) asm volatile("" : "+v"(bias));
  // First k-step of an S^T chain: acc = bias + K.Q^T.  C is either the resident bias tuple or the MFMA's own destination
  // registers initialised in place (C = D), so the chain never needs a second 16-register tuple.
  auto mfma_s_first = [&](const v4i a, const v4i b) __attribute__((always_inline)) -> v16i {
    if constexpr (BIAS_RESIDENT) {
      return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, bias, 0, 0, 0);
    } else {
      v16i acc = bias;
      asm volatile("" : "+v"(acc));  // the 16 moves land in the accumulator itself
      return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
    }
  };

  // S^T = K . Q^T for one tile (2 x 32 keys x 32 query rows) out of LDS buffer `kbuf`
  auto qk = [&](const int kbuf, v16i (&s)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const v4i a = *reinterpret_cast<const v4i*>(k_rd[ks] + (kbuf * KBYTES + mt * 32 * D));
        s[mt] = ks == 0 ? mfma_s_first(a, qf[ks]) : __builtin_amdgcn_mfma_i32_32x32x32_i8(a, qf[ks], s[mt], 0, 0, 0);
      }
  };
  // dequantisation scales of tile j: …sm80.cu:131, 4 per 64 keys, index (c%8)/2 = 2*hh + ((reg&3)>>1)
  // wave-uniform address: the scales of a tile come through the scalar cache (s_load_dwordx4, lgkmcnt), not through
  // vmcnt where they would queue behind the tile DMA.  The lane-half select is an fma with a zeroed partner
  // (x*q + z*0 is exactly x*q) instead of two v_mov + v_cndmask per scale: SGPR operands feed the VALU directly.
  float qsc_lo = 0.f, qsc_hi = 0.f;  // = hh ? (0, qsc) : (qsc, 0), set once the Q scale is known (prologue)
  // (PAGED: out of the scale row of page `page`, [P, Hk, tpp * (4 | 1)]: the same load at the same depth)
  auto load_kscales = [&](const int j, const int page = 0) __attribute__((always_inline)) -> float4 {
    if constexpr (PAGED) {
      const float* sp = pg_ks + (int64_t)page * p.ks_b + ((sk_t0 + j) & pg_tmask) * p.ks_t;
      if constexpr (KTHREAD) return uniform_load4(sp);
      else return make_float4(uniform_load1(sp), 0.f, 0.f, 0.f);
    } else {
    if constexpr (KTHREAD) return uniform_load4(ksp + j * p.ks_t);
    else return make_float4(uniform_load1(ksp + j * p.ks_t), 0.f, 0.f, 0.f);
    }
  };
  auto scales_from = [&](const float4 kk, float& sc0, float& sc1) __attribute__((always_inline)) {
    if constexpr (KTHREAD) {
      sc0 = __builtin_fmaf(kk.z, qsc_hi, kk.x * qsc_lo);
      sc1 = __builtin_fmaf(kk.w, qsc_hi, kk.y * qsc_lo);
    } else {
      sc0 = sc1 = qsc * kk.x;
    }
  };
  auto tile_scales = [&](const int j, float& sc0, float& sc1, const int page = 0) __attribute__((always_inline)) {
    scales_from(load_kscales(j, page), sc0, sc1);
  };
  // which of the lane's 32 keys of tile j may be attended: bit 16*mt+e.  Sequence end, causal diagonal and the
  // caller's bool attn_mask (False = masked; the reference adds -1e6, which is the same for every row that keeps
  // at least one key; rows with no allowed key at all are undefined there -- they depend on its tile skipping).
  // attn_mask exists only on the non-causal 16-bit-PV operator (fp16 or bf16 V; the reference converts a bf16 V to fp16
  // for masked calls as well, core.py:289-290)
  constexpr bool CAN_MASK = HAS_MASK;  // separate instantiation: the mask bookkeeping must not cost the main variants registers
  const uint8_t* mrow = nullptr;
  if constexpr (CAN_MASK)
    if (p.mask) mrow = p.mask + ((int64_t)b * p.msb + (int64_t)h * p.msh + (int64_t)rowc * p.msm) * (p.mask_kind == 1 ? 1 : 2);
  struct __attribute__((packed)) u32_unaligned { uint32_t v; };
  struct __attribute__((packed)) u64_unaligned { uint64_t v; };
  auto allow_bits = [&](const int j) __attribute__((always_inline)) -> uint32_t {
    const int n0 = j << 6;
    uint32_t bits = 0;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int kv0 = n0 + 32 * mt + 8 * g4 + 4 * hh;  // the lane's keys come in runs of 4: registers 4*g4 .. 4*g4+3
        uint32_t run = 0;                                 // bit i: key kv0+i allowed
#pragma unroll
        for (int i = 0; i < 4; ++i) run |= (((kv0 + i) < N_ && !(CAUSAL && (kv0 + i) > row)) ? 1u : 0u) << i;
        if constexpr (CAN_MASK) {
          if (p.mask_kind == 1 && run) {
            uint32_t mb = 0;
            if (p.msn == 1 && kv0 + 3 < N_) {  // 4 mask bytes in one (unaligned) dword
              const uint32_t w = reinterpret_cast<const u32_unaligned*>(mrow + kv0)->v;
#pragma unroll
              for (int i = 0; i < 4; ++i) mb |= (((w >> (8 * i)) & 0xffu) ? 1u : 0u) << i;
            } else {
#pragma unroll 1
              for (int i = 0; i < 4; ++i)
                if (kv0 + i < N_) mb |= (mrow[(int64_t)(kv0 + i) * p.msn] ? 1u : 0u) << i;
            }
            run &= mb;
          }
        }
        bits |= run << (16 * mt + 4 * g4);
      }
    return bits;
  };
  // sequence end and causal diagonal (the kernels without attn_mask): register e of block mt holds key
  // 64*j + 32*mt + (e&3) + 8*(e>>2) + 4*hh, allowed iff <= min(N-1, row): one compare against a per-lane limit
  auto mask_limit = [&](const int j, v16i (&s)[2]) __attribute__((always_inline)) {
    // (causal split-KV under `if constexpr`: named in the expression of the others, lim_l is captured by this lambda in every
    //  kernel, and the FP8 head_dim-64 block-sparse kernels came out with two scalar moves in another order)
    int lim;
    if constexpr (CAUSAL && SPLITKV) lim = min(N_ - 1, lim_l) - (j << 6) - 4 * hh_l;
    else lim = min(N_ - 1, CAUSAL ? row_l : 0x7fffffff) - (j << 6) - 4 * hh_l;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) s[mt][e] = (32 * mt + (e & 3) + 8 * (e >> 2) <= lim) ? s[mt][e] : kMaskedI;
  };
  auto mask_scores = [&](const uint32_t bits, v16i (&s)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) s[mt][e] = ((bits >> (16 * mt + e)) & 1u) ? s[mt][e] : kMaskedI;
  };
  // additive attn_mask: the score registers are rewritten in place with the fp32 base-2 logits
  // t = S*scale + mask (masked / out-of-range keys: -1e6 as in the reference, attn_qk_int8_per_block.py:40-43)
  const bool fmask = CAN_MASK && p.mask_kind >= 2;
  auto to_float_logits = [&](const int j, const uint32_t bits, v16i (&s)[2], const float sc0, const float sc1)
      __attribute__((always_inline)) {
    const int n0 = j << 6;
    const uint16_t* mrow16 = reinterpret_cast<const uint16_t*>(mrow);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int kv0 = n0 + 32 * mt + 8 * g4 + 4 * hh;
        uint16_t raw[4] = {0, 0, 0, 0};
        if (p.msn == 1 && kv0 + 3 < N_) {  // 4 mask values in one (unaligned) 8-byte load
          const uint64_t w = reinterpret_cast<const u64_unaligned*>(mrow16 + kv0)->v;
#pragma unroll
          for (int i = 0; i < 4; ++i) raw[i] = (uint16_t)(w >> (16 * i));
        } else {
#pragma unroll 1
          for (int i = 0; i < 4; ++i)
            if (kv0 + i < N_) raw[i] = mrow16[(int64_t)(kv0 + i) * p.msn];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = 4 * g4 + i;
          const float sc = (e & 2) ? sc1 : sc0;
          const float t = __builtin_fmaf(__int_as_float(s[mt][e]), sc, -kBiasF * sc);
          float mv = -1.0e6f;
          if ((bits >> (16 * mt + e)) & 1u) mv = p.mask_kind == 3 ? bf16_bits_to_f32(raw[i]) : f16_bits_to_f32(raw[i]);
          s[mt][e] = __float_as_int(t + mv);
        }
      }
  };
  auto row_max_f = [&](const v16i (&s)[2]) __attribute__((always_inline)) -> float {
    float mx = __int_as_float(s[0][0]);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) mx = fmaxf(mx, __int_as_float(s[mt][e]));
    return swap_max(mx);
  };
  // row max of the logits of one tile, from the raw integers (scales are positive): v_max3_i32 + 1 cvt/group
  auto row_max = [&](const v16i (&s)[2], const float sc0, const float sc1) __attribute__((always_inline)) -> float {
    int mxa = s[0][0], mxb = s[0][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if (e & 2) mxb = max(mxb, s[mt][e]); else mxa = max(mxa, s[mt][e]);
      }
    // the biased integers are the floats 12582912 + S: one v_sub_f32 recovers S exactly (no v_cvt_f32_i32)
    float mx;
    if constexpr (KTHREAD) mx = max_raw((__int_as_float(mxa) - kBiasF) * sc0, (__int_as_float(mxb) - kBiasF) * sc1);
    else mx = (__int_as_float(max(mxa, mxb)) - kBiasF) * sc0;
    return swap_max(mx);
  };
  // lazy rescale (attn_utils.cuh:354-458 rescales every tile; here only when some row's max grew by more than
  // kLazyThr, so p <= 2^kLazyThr -- harmless in fp16/fp32; m_run stays exact for the LSE)
  // fp8: p carries the reference's exponent offset (attn_utils.cuh:30,379: m tracked as t - 8.807 so p <= 448 = e4m3
  // max); the lazy threshold is taken out of that headroom so p <= 2^(kLazyThr + kPOff) = 448 still holds.
  constexpr float kLazyThr = PV_FP8 ? 3.0f : 6.0f;
  constexpr float kPOff = PV_FP8 ? 8.807f - 3.0f : 0.f;
  float m_thr = m_run + kLazyThr;  // kept in a register: the comparison runs every tile, the update almost never
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
  // PVSKIP: the wave leaves out the softmax and P.V of the tile at list position `pos` (row maximum `mx`) iff pos > 0 and
  // on every row < M the tile's maximum lies at least the threshold below the running reference maximum.  Asked AFTER
  // maybe_rescale(mx): a row whose maximum grew has m_run = mx there and vetoes.  Wave uniform.
  auto pv_skip = [&](const int pos, const float mx) __attribute__((always_inline)) -> bool {
    if constexpr (PVSKIP) {
      // (the position is made opaque: seeing that `pos > 0` holds from the second tile on, hipcc peels the first round of
      //  the unrolled fast loops -- a second copy of the hand-placed stream with a register assignment of its own)
      int po = pos;
      asm volatile("" : "+s"(po));
      return po > 0 && (__builtin_amdgcn_ballot_w64(mx > m_run - pv_thr) & pv_rows) == 0;
    } else {
      return false;
    }
  };
  // P pair -> two packed 16-bit values in the element type of V (RNE both), and the P.V MFMA of that type
  auto pack_p = [&](const v2f two) __attribute__((always_inline)) -> v2h {
    if constexpr (V_BF16) return __builtin_bit_cast(v2h, __builtin_convertvector(two, v2bf));  // v_cvt_pk_bf16_f32
    else return __builtin_convertvector(two, v2h);                                              // v_cvt_pk_f16_f32 (fp16_rn)
  };
  auto pv_mfma = [&](const v8h a, const v8h b, const v16f c) __attribute__((always_inline)) -> v16f {
    if constexpr (V_BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  };
  // p = exp2(t - m) and O^T += V^T . P^T
  uint32_t bits_cur = 0xffffffffu;  // allow mask of tile j (attn_mask loop only)
  auto softmax_pv = [&](const int j, const int vbuf, const v16i (&s)[2], const float sc0, const float sc1,
                        auto masked_tag) __attribute__((always_inline)) {
    constexpr bool MASKED = decltype(masked_tag)::value;
    const float c0 = __builtin_fmaf(-kBiasF, sc0, kPOff - m_run), c1 = __builtin_fmaf(-kBiasF, sc1, kPOff - m_run);
    auto prob = [&](const int mt, const int e) __attribute__((always_inline)) -> float {
      const bool g1 = (e & 2) != 0;
      float pv;
      if (MASKED && fmask) {
        pv = __builtin_amdgcn_exp2f(__int_as_float(s[mt][e]) - m_run + kPOff);  // registers hold fp32 logits
      } else {
        pv = __builtin_amdgcn_exp2f(__builtin_fmaf(__int_as_float(s[mt][e]), g1 ? sc1 : sc0, g1 ? c1 : c0));
      }
      return pv;
    };
    if constexpr (!PV_FP8) {
      // quarters of 16 keys, each followed by its PV MFMAs
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int sq = 0; sq < 2; ++sq) {
          v8h pf;
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            v2f pp = {prob(mt, 8 * sq + e), prob(mt, 8 * sq + e + 1)};
            const v2h ph = pack_p(pp);
            pf[e] = ph[0];
            pf[e + 1] = ph[1];
            if constexpr (!MROW) {
              l_run += pp[0];
              l_run += pp[1];
            }
          }
          if constexpr (MROW) rowsum8(pf);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            const char* base = v_rd[dt] + (vbuf * VBYTES + (32 * mt + 16 * sq) * (2 * D));
            const v4s_vs lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_vs*)(base));
            const v4s_vs hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) v4s_vs*)(base + 8 * (2 * D)));
            v8h a;
            a.s0123 = __builtin_bit_cast(v4h, lo);
            a.s4567 = __builtin_bit_cast(v4h, hi);
            acc_o[dt] = pv_mfma(a, pf, acc_o[dt]);
          }
        }
    } else {
      // all 64 keys of the tile in one K=64 MFMA per d tile; P^T bytes in accumulator order j = 16*mt + reg
      v8i pb;
      float psum = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        const int mt = w >> 2, e0 = 4 * (w & 3);
        const float p0 = prob(mt, e0), p1 = prob(mt, e0 + 1), p2 = prob(mt, e0 + 2), p3 = prob(mt, e0 + 3);
        psum += p0; psum += p1; psum += p2; psum += p3;
        int pk = 0;
        if constexpr (D == 128) asm volatile("" : "=v"(pk));  // (no v_mov for the `old` operand: see the hand-placed stream)
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(p0, p1, pk, false);  // OCP e4m3, RNE (e4m3_rn_satfinite)
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(p2, p3, pk, true);
        pb[w] = pk;
      }
      l_run += psum;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int base = vbuf * VBYTES + dt * 32 * 64;
        const v4i lo = *reinterpret_cast<const v4i*>(v_rd8[0] + base);
        const v4i hi = *reinterpret_cast<const v4i*>(v_rd8[1] + base);
        v8i a;
        a.s0123 = lo;
        a.s4567 = hi;
        // cbsz = blgp = 0: both operands e4m3; E8M0 block scales 127 = 2^0
        acc_o[dt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, pb, acc_o[dt], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
      }
    }
  };

  // ---- software pipeline.  LDS: K(j) in K buffer j&1, V(j) in V buffer j&1.  During iteration j the wave
  //      computes S(j+1) = K(j+1).Q^T (MFMA) while it exponentiates S(j) (VALU) and accumulates P(j).V(j);
  //      K(j+2) and V(j+1) are copied global -> LDS during the iteration (LDS-DMA, drained in front of the barrier).
  //   [0, n_fast)           tiles j and j+1 both unmasked: branch-free body
  //   [n_fast, wave_tiles)  the wave's last tiles (a successor that may need masking; the final tile): run-time ring slots
  //   [wave_tiles, ntiles)  causal only: this wave is done but still stages tiles for its workgroup
  // Every wave executes the same number of barriers.
  int n_plain = wave_tiles;
  if constexpr (SPARSE) {  // the list ascends: only its last entry can be the ragged tile
    if ((N_ & 63) && tile_at(ntiles - 1) == (N_ >> 6)) n_plain = ntiles - 1;
  } else {
    if (N_ & 63) n_plain = min(n_plain, N_ >> 6);
  }
  // tile j needs no mask iff 64*j+63 <= q0 (causal split-KV: <= the limit of the wave's first row)
  if constexpr (CAUSAL && SPLITKV) n_plain = min(n_plain, (max(sk_tok0 + sk_off, -1) + 1) >> 6);
  else if constexpr (CAUSAL) n_plain = min(n_plain, max(0, (q0 + 1) >> 6));
  const int n_fast = (CAN_MASK && p.mask) ? 0 : max(0, min(n_plain - 1, wave_tiles - 1));  // attn_mask: all tiles generic

  // tile copies a wave issues per iteration (full tiles): the unit of the counted waits of the four-slot ring
  constexpr int NDMA = KC + VC;
  static_assert(RING == 2 || (KC * T == 64 * KCH && VC * T == VROWS * VCH), "four-slot ring: every wave copies full shares");
  const int last_tile = ntiles - 1;
  // list position of a read-ahead -> key tile.  Dense: clamped to the last tile; block-sparse: the padded list is read blindly
  auto ahead = [&](const int pos) __attribute__((always_inline)) -> int {
    if constexpr (SPARSE) return tile_at(pos); else return min(pos, last_tile);
  };
  // PAGED: the page of the tile at position `pos` of the range, the position clamped like every read-ahead (dense: nothing)
  auto page_at = [&](const int pos) __attribute__((always_inline)) -> int {
    if constexpr (PAGED) return uniform_load_i32(pg_row + ((sk_t0 + min(pos, last_tile)) >> p.bt_shift)); else return 0;
  };
  if constexpr (PAGED) {  // the pages of the first five tiles, requested together: one scalar round trip in front of the first copies
#pragma unroll
    for (int i = 0; i < 5; ++i) bs_first[i] = page_at(i);
  }
  if constexpr (SPARSE) {
    if constexpr (RING == 2) {
      dma_k(bs_first[0], 0);
      load_v(bs_first[0], 0);
      if (ntiles > 1) dma_k(bs_first[1], 1);
      prepare_q();
      dma_wait_all();
    } else {
      dma_k(bs_first[0], 0);
      load_v(bs_first[0], 0);
      dma_k(bs_first[1], 1);
      load_v(bs_first[1], 1);
      dma_k(bs_first[2], 2);
      load_v(bs_first[2], 2);
      dma_k(bs_first[3], 3);
      prepare_q();
      dma_wait_keep<2 * NDMA>();
    }
  } else if constexpr (RING == 2) {
    dma_k(0, 0, bs_first[0]);
    load_v(0, 0, bs_first[0]);
    if (ntiles > 1) dma_k(1, 1, bs_first[1]);
    prepare_q();
    dma_wait_all();
  } else {
    // K(0..3) and V(0..2), clamped to the last tile so that every wave issues the same number of copies whatever the
    // sequence length (a clamped copy re-loads the last tile into a slot nobody reads any more); only K(0), V(0), K(1)
    // are needed now, the rest keeps flying
    dma_k(0, 0, bs_first[0]);
    load_v(0, 0, bs_first[0]);
    dma_k(min(1, last_tile), 1, bs_first[1]);
    load_v(min(1, last_tile), 1, bs_first[1]);
    dma_k(min(2, last_tile), 2, bs_first[2]);
    load_v(min(2, last_tile), 2, bs_first[2]);
    dma_k(min(3, last_tile), 3, bs_first[3]);
    prepare_q();
    dma_wait_keep<2 * NDMA>();
  }
  qsc_lo = hh ? 0.f : qsc;
  qsc_hi = hh ? qsc : 0.f;
  __syncthreads();

  if constexpr (HAS_MASK) {
    // attn_mask instantiation: plain serial loop (K and V one tile ahead), every tile through the masked body.
    // A tile in which this wave's 32 rows keep no key is skipped (the reference skips all-False 128x64 tiles,
    // attn_qk_int8_per_block.py:38-39).
    v16i s_cur[2];
    float sc0, sc1;
    for (int j = 0; j < ntiles; ++j) {
      const int buf = j & 1;
      if (j + 1 < ntiles) {
        if (j > 0) dma_k(j + 1, buf ^ 1);  // K(1) was copied by the prologue
        load_v(j + 1, buf ^ 1);
      }
      bits_cur = allow_bits(j);
      if (__builtin_amdgcn_ballot_w64(bits_cur != 0) != 0) {
        tile_scales(j, sc0, sc1);
        qk(buf, s_cur);
        float mx;
        if (fmask) { to_float_logits(j, bits_cur, s_cur, sc0, sc1); mx = row_max_f(s_cur); }
        else { mask_scores(bits_cur, s_cur); mx = row_max(s_cur, sc0, sc1); }
        maybe_rescale(mx);
        softmax_pv(j, buf, s_cur, sc0, sc1, std::true_type{});
      }
      dma_wait_all();
      __syncthreads();
    }
  } else {
  v16i s_cur[2], s_nxt[2];
  float sc0, sc1, mx_cur;
  qk(0, s_cur);
  // Every wave reads ALL 64 rows of K buffer 0 for S(0) above, and iteration 0 below re-fills that buffer with K(2)
  // (each wave DMA-writes its own 1 KiB slice).  Later iterations are ordered by the barrier that closes the previous
  // one; this first re-fill needs its own: without it a wave that is held back between the prologue barrier and its
  // K(0) fragment reads (three waves per SIMD: the youngest wave can starve for longer than an L2 round trip) computes
  // S(0) from a mix of K(0) and K(2) rows -- one wrong 32-row wave, the same wrong value every time
  // (profiles/r02_race_evidence.md).
  __syncthreads();
  tile_scales(SPARSE ? bs_first[0] : 0, sc0, sc1, bs_first[0]);
  // a plain tile 0 needs no mask (64 compare + select instructions per wave); the causal head_dim-64 variants keep it
  // unconditional -- under the branch they need 170 registers, two over the three-waves-per-SIMD line
  if (CAUSAL || n_plain <= 0) mask_limit(SPARSE ? bs_first[0] : 0, s_cur);
  mx_cur = row_max(s_cur, sc0, sc1);

  // fast loop, unrolled by two so that S(j) / S(j+1) swap roles without register copies
  float4 kk_nxt = load_kscales(SPARSE ? bs_first[1] : min(1, ntiles - 1), bs_first[1]);
  // block-sparse: the key tiles at list positions j+1 .. j+RING, in SGPRs.  Iteration j requests the entry of position
  // j+RING+1 next to the scale load and shifts it in at its end, so the tile of every copy and of the scale load of
  // position j+2 is known a whole iteration before it is used: no scalar round trip in front of a copy or a K-fragment wait.
  // PAGED: the same window holds the PAGES of the tiles min(j+1 .. j+RING, last_tile), requested and shifted the same way.
  int bw1 = bs_first[1], bw2 = bs_first[2], bw3 = bs_first[3], bw4 = bs_first[4];
  (void)bw1; (void)bw2; (void)bw3; (void)bw4;
  int k_slot = 0, v_slot = 0;  // slots the LDS read pointers point at (moved by the run-time-slot tiles only)
  // NEXT (second tag): what follows tile j for this wave.
  //   0  a plain tile: the fast loops.  Ring slots are compile-time (R = j % RING), every LDS offset an immediate.
  //   1  a tile that may need masking (sequence end, causal diagonal), 2  nothing (the wave's last tile): the remaining
  //      tiles of a wave run through the SAME hand-placed stream with run-time ring slots (a few address adds) -- the
  //      compiler-scheduled body is 1.6x slower per tile, 5-7 % of a short causal sequence.
  auto fast_iter = [&](auto par_tag, auto next_tag, const int j, v16i (&sa)[2], v16i (&sb)[2], float& a0, float& a1, float& b0,
                       float& b1) __attribute__((always_inline)) {
    constexpr int R = decltype(par_tag)::value;  // j % RING, static so every LDS offset is an immediate
    constexpr int NEXT = decltype(next_tag)::value;
    constexpr bool DYN = NEXT != 0;
    // slots of K(j+1), V(j), K(j+RING), V(j+RING-1)
    const int K_RD = DYN ? (j + 1) % RING : (R + 1) % RING, V_RD = DYN ? j % RING : R, K_WR = V_RD,
              V_WR = DYN ? (j + RING - 1) % RING : (R + RING - 1) % RING;
    // The first K fragment of S(j+1) is read BEFORE the tile copies are issued: the first S MFMA needs it at once, and the
    // copies are inline asm with a memory clobber, so the compiler cannot hoist the read across them itself (+0.2..0.8 %).
    // scales of tile j+1 were fetched during the previous iteration; those of tile j+2 are fetched first thing here: the
    // scalar load shares lgkmcnt with the LDS reads, so it must be in flight long before the first wait on a K fragment
    // (left to hipcc it is issued right in front of that wait and every iteration pays a scalar-cache round trip)
    if constexpr (DYN) {
      // run-time slots without extra address registers: the read pointers themselves move to the slots of this tile (the
      // fast loops, which need them at the region base, are over) and every offset below stays an immediate
      if constexpr (NEXT != 2) {
        const int dk = (K_RD - k_slot) * KBYTES;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) k_rd[ks] += dk;
        k_slot = K_RD;
      }
      const int dv = (V_RD - v_slot) * VBYTES;
      if constexpr (PV_FP8) { v_rd8[0] += dv; v_rd8[1] += dv; }
      else {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) v_rd[dt] += dv;
      }
      v_slot = V_RD;
    }
    v4i kf_early = qf[0];
    int bw_in = RING == 2 ? bw2 : bw4;  // block-sparse: the entry that enters the window (the wave's last tile: none)
    if constexpr (NEXT != 2) {
      scales_from(kk_nxt, b0, b1);
      kk_nxt = load_kscales(SPARSE ? bw2 : min(j + 2, ntiles - 1), bw2);
      if constexpr (SPARSE) bw_in = tile_at(j + RING + 1);
      if constexpr (PAGED) bw_in = page_at(j + RING + 1);
      kf_early = *reinterpret_cast<const v4i*>(k_rd[0] + (DYN ? 0 : K_RD * KBYTES));
    }
    __builtin_amdgcn_sched_barrier(0);
    maybe_rescale(mx_cur);
    if constexpr (RING == 2) {
      if (j + 2 < ntiles) dma_k(SPARSE ? bw2 : j + 2, K_WR, bw2);
      if (!DYN || j + 1 < ntiles) load_v(SPARSE ? bw1 : j + 1, V_WR, bw1);
    } else {
      dma_k(SPARSE ? bw4 : min(j + RING, last_tile), K_WR, bw4);
      load_v(SPARSE ? bw3 : min(j + RING - 1, last_tile), V_WR, bw3);
    }
    bool skip = false;
    if constexpr (PVSKIP) skip = pv_skip(j, mx_cur);
    if (skip) {
      // PVSKIP, a negligible tile: only what S(j+1) needs -- its K fragments, its MFMAs, the sequence-end mask and the row
      // maximum.  No V fragment read, no exponential, no P.V MFMA; m_run, the row sums and O stay as they are.  The copies
      // above and the wait and barrier below are those of a computing wave.
      if constexpr (PVSKIP) {
        ++n_skipped;
        if constexpr (NEXT != 2) {
          constexpr int NS = 2 * KS;
          const int kb = DYN ? 0 : K_RD * KBYTES;
          v4i kf = kf_early;
#pragma unroll
          for (int i = 0; i < NS; ++i) {
            const int mt = i / KS, ks = i % KS;
            v4i kn = kf;
            if (i + 1 < NS) kn = *reinterpret_cast<const v4i*>(k_rd[(i + 1) % KS] + (kb + ((i + 1) / KS) * 32 * D));
            sb[mt] = ks == 0 ? mfma_s_first(kf, qf[ks]) : __builtin_amdgcn_mfma_i32_32x32x32_i8(kf, qf[ks], sb[mt], 0, 0, 0);
            kf = kn;
          }
          if constexpr (NEXT == 1) { if (j + 1 >= n_plain) mask_limit(SPARSE ? bw1 : j + 1, sb); }
          mx_cur = row_max(sb, b0, b1);
        }
      }
    } else if constexpr (PV_FP8) {
      // Hand-placed stream, FP8 PV.  The K = 64 MFMA consumes the P of the whole tile, so all of P(j) precedes the P.V
      // MFMAs; left alone hipcc emits ~110 softmax VALU instructions with the matrix pipe idle and then the 12 MFMAs in
      // one cluster.  Here: the S(j+1) MFMAs are spread through the computation of the eight P words (4 keys each:
      // 4 fma, 4 exp2, 2 cvt_pk_fp8; the row-sum adds trail by one word), the V^T fragments are read while the last
      // words are computed, and the four P.V MFMAs run beside the row max of S(j+1).
      constexpr int NS = 2 * KS;       // S MFMAs per tile
      constexpr int WPS = 8 / NS;      // P words per S MFMA (1 at head_dim 128, 2 at 64)
      const int kb = DYN ? 0 : K_RD * KBYTES, vb = DYN ? 0 : V_RD * VBYTES;  // slot offsets (DYN: the pointers were moved)
      const float c0 = __builtin_fmaf(-kBiasF, a0, kPOff - m_run), c1 = __builtin_fmaf(-kBiasF, a1, kPOff - m_run);
      auto k_frag = [&](const int i) __attribute__((always_inline)) -> v4i {
        return *reinterpret_cast<const v4i*>(k_rd[i % KS] + (kb + (i / KS) * 32 * D));
      };
      auto s_step = [&](const int i, const v4i a) __attribute__((always_inline)) {
        const int mt = i / KS, ks = i % KS;
        sb[mt] = ks == 0 ? mfma_s_first(a, qf[ks]) : __builtin_amdgcn_mfma_i32_32x32x32_i8(a, qf[ks], sb[mt], 0, 0, 0);
      };
      auto v_frag8 = [&](const int dt) __attribute__((always_inline)) -> v8i {
        const int base = vb + dt * 32 * 64;
        v8i a;
        a.s0123 = *reinterpret_cast<const v4i*>(v_rd8[0] + base);
        a.s4567 = *reinterpret_cast<const v4i*>(v_rd8[1] + base);
        return a;
      };
      v8i pb;
      float pend[4], psum = 0.f;
      auto p_word = [&](const int w) __attribute__((always_inline)) {
        const int mt = w >> 2, e0 = 4 * (w & 3);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool g1 = ((e0 + i) & 2) != 0;
          pend[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(__int_as_float(sa[mt][e0 + i]), g1 ? a1 : a0, g1 ? c1 : c0));
        }
        // (the first convert's `old` operand is a register nobody has written: both halves of the dword are produced by the two
        //  converts, and a literal 0 there costs a v_mov_b32 per P word -- 8 of ~166 vector instructions per tile)
        int pk = 0;
        if constexpr (D == 128) asm volatile("" : "=v"(pk));  // (head_dim 64: the variants at the 168-register line spill with it)
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(pend[0], pend[1], pk, false);  // OCP e4m3, RNE
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(pend[2], pend[3], pk, true);
        pb[w] = pk;
      };
      auto p_sum = [&]() __attribute__((always_inline)) {
        psum += pend[0]; psum += pend[1]; psum += pend[2]; psum += pend[3];
      };
#define SAGE_FENCE() __builtin_amdgcn_sched_barrier(0)
      v4i kf = kf_early;
      v8i vf[DT];
      int si = 0;
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        if (NEXT != 2 && w % WPS == 0) {
          s_step(si, kf);
          if (si + 1 < NS) kf = k_frag(si + 1);
          ++si;
        }
        if (w > 0) p_sum();
        p_word(w);
        if (w == 6) vf[0] = v_frag8(0);
        if (w == 7 && DT > 1) vf[1] = v_frag8(1);
        SAGE_FENCE();
      }
      p_sum();
      l_run += psum;
      // P.V beside the row max of S(j+1)
      if constexpr (NEXT == 1) { if (j + 1 >= n_plain) mask_limit(SPARSE ? bw1 : j + 1, sb); }
      int mxa = sb[0][0], mxb = sb[0][2];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        if (dt + 2 < DT) vf[dt + 2] = v_frag8(dt + 2);
        acc_o[dt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf[dt], pb, acc_o[dt], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
        if constexpr (NEXT != 2) {
#pragma unroll
          for (int idx = dt * (32 / DT); idx < (dt + 1) * (32 / DT); ++idx) {
            const int mt = idx >> 4, e = idx & 15;
            if (e & 2) mxb = max(mxb, sb[mt][e]); else mxa = max(mxa, sb[mt][e]);
          }
          asm volatile("" : "+v"(mxa), "+v"(mxb));
        }
        SAGE_FENCE();
      }
#undef SAGE_FENCE
      if constexpr (NEXT != 2) {
        float mx;
        if constexpr (KTHREAD) mx = max_raw((__int_as_float(mxa) - kBiasF) * b0, (__int_as_float(mxb) - kBiasF) * b1);
        else mx = (__int_as_float(max(mxa, mxb)) - kBiasF) * b0;
        mx_cur = swap_max(mx);
      }
    } else {
      // Hand-placed instruction stream (fp16 PV).  The wave issues in order and an MFMA that finds the matrix pipe
      // busy blocks the VALU instructions behind it, so what counts is what sits BETWEEN consecutive MFMAs: about
      // 24 cycles of vector issue hide beside a 32-cycle MFMA (tools/issue_cost.hip).  Left to itself hipcc emits the
      // S(j+1) MFMAs as one burst, P.V MFMAs with nothing but LDS reads between them, and the row sums / row max as a
      // VALU-only tail.  Here the tile is cut into quarters of 16 keys: P of quarter q+1 is computed beside the P.V
      // MFMAs of quarter q, the S(j+1) MFMAs are spread between them, V^T fragments are read one quarter ahead, and
      // the row max of S(j+1) runs beside the last quarter's MFMAs.  sched_barrier(0) pins each group.
      constexpr int NS = 2 * KS, SPR = NS / 4;  // S MFMAs per tile / per region
      constexpr int PPG = 4 / DT;               // P pairs computed beside one P.V MFMA
      const int kb = DYN ? 0 : K_RD * KBYTES, vb = DYN ? 0 : V_RD * VBYTES;  // slot offsets (DYN: the pointers were moved)
      const float c0 = __builtin_fmaf(-kBiasF, a0, kPOff - m_run), c1 = __builtin_fmaf(-kBiasF, a1, kPOff - m_run);
      auto k_frag = [&](const int i) __attribute__((always_inline)) -> v4i {
        return *reinterpret_cast<const v4i*>(k_rd[i % KS] + (kb + (i / KS) * 32 * D));
      };
      auto v_frag = [&](const int q, const int dt) __attribute__((always_inline)) -> v8h {
        const char* base = v_rd[dt] + (vb + 16 * q * (2 * D));
        const v4s_vs lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_vs*)(base));
        const v4s_vs hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_vs*)(base + 8 * (2 * D)));
        v8h a;
        a.s0123 = __builtin_bit_cast(v4h, lo);
        a.s4567 = __builtin_bit_cast(v4h, hi);
        return a;
      };
      auto s_step = [&](const int i, const v4i a) __attribute__((always_inline)) {
        const int mt = i / KS, ks = i % KS;
        sb[mt] = ks == 0 ? mfma_s_first(a, qf[ks]) : __builtin_amdgcn_mfma_i32_32x32x32_i8(a, qf[ks], sb[mt], 0, 0, 0);
      };
      float pp[8];  // unrounded p of the quarter in flight (row-sum operands)
      auto p_pair = [&](const int q, const int pr, v8h& pf) __attribute__((always_inline)) {
        const int mt = q >> 1, e = 8 * (q & 1) + 2 * pr;
        const bool g1 = (e & 2) != 0;
        const float sc = g1 ? a1 : a0, cc = g1 ? c1 : c0;
        v2f two = {__builtin_amdgcn_exp2f(__builtin_fmaf(__int_as_float(sa[mt][e]), sc, cc)),
                   __builtin_amdgcn_exp2f(__builtin_fmaf(__int_as_float(sa[mt][e + 1]), sc, cc))};
        const v2h ph = pack_p(two);
        pf[2 * pr] = ph[0];
        pf[2 * pr + 1] = ph[1];
        if constexpr (!MROW) {
          pp[2 * pr] = two[0];
          pp[2 * pr + 1] = two[1];
        }
      };
      // row sum of pair `pr` of the quarter whose packed P is `vec` (MROW: one MFMA per quarter, after its last pair)
      auto p_sum = [&](const int pr, const v8h& vec) __attribute__((always_inline)) {
        if constexpr (MROW) {
          if (pr == 3) rowsum8(vec);
        } else {
          l_run += pp[2 * pr];
          l_run += pp[2 * pr + 1];
        }
      };
#define SAGE_FENCE() __builtin_amdgcn_sched_barrier(0)
      v4i kf = kf_early;
      // head_dim 64: K fragments are read TWO S MFMAs ahead (two registers in flight; four S MFMAs per tile, one per region,
      // so one-ahead left the read ~70 cycles): C2 +0.75 %; head_dim 128 (eight S MFMAs, two per region): -0.3 % -> not there.
      constexpr bool KPREF2 = D == 64;
      v4i kfq[2] = {kf_early, kf_early};
      if constexpr (KPREF2 && NEXT != 2) kfq[1] = k_frag(1);
      v8h vf[DT], vn[DT], pf, pn;
      // region 0: P(quarter 0) beside the first S MFMAs; V^T fragments of quarter 0
#pragma unroll
      for (int g = 0; g < SPR; ++g) {
        if constexpr (NEXT != 2) {
          if constexpr (KPREF2) {
            s_step(g, kfq[g & 1]);
            if (g + 2 < NS) kfq[g & 1] = k_frag(g + 2);
          } else {
            s_step(g, kf);
            kf = k_frag(g + 1);
          }
        }
#pragma unroll
        for (int dt = g * (DT / SPR); dt < (g + 1) * (DT / SPR); ++dt) vf[dt] = v_frag(0, dt);
#pragma unroll
        for (int pr = g * (4 / SPR); pr < (g + 1) * (4 / SPR); ++pr) {
          if (pr > 0) p_sum(pr - 1, pf);
          p_pair(0, pr, pf);
        }
        SAGE_FENCE();
      }
      // regions 1..3: P.V of quarter q-1 | P(quarter q) | S MFMAs | V^T fragments of quarter q
      int si = SPR;
#pragma unroll
      for (int q = 1; q < 4; ++q) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          acc_o[dt] = pv_mfma(vf[dt], pf, acc_o[dt]);
          vn[dt] = v_frag(q, dt);
#pragma unroll
          for (int pr = dt * PPG; pr < (dt + 1) * PPG; ++pr) {
            p_sum(pr == 0 ? 3 : pr - 1, pr == 0 ? pf : pn);  // the pair computed one step earlier (pair 3 of the previous quarter first)
            p_pair(q, pr, pn);
          }
          SAGE_FENCE();
          if (NEXT != 2 && (dt + 1) % (DT / SPR) == 0) {
            if constexpr (KPREF2) {
              s_step(si, kfq[si & 1]);
              if (si + 2 < NS) kfq[si & 1] = k_frag(si + 2);
            } else {
              s_step(si, kf);
              if (si + 1 < NS) kf = k_frag(si + 1);
            }
            ++si;
            SAGE_FENCE();
          }
        }
        pf = pn;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) vf[dt] = vn[dt];
      }
      // tail: P.V of quarter 3 beside the row max of S(j+1)
      p_sum(3, pf);
      if constexpr (NEXT == 1) { if (j + 1 >= n_plain) mask_limit(SPARSE ? bw1 : j + 1, sb); }
      int mxa = sb[0][0], mxb = sb[0][2];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        acc_o[dt] = pv_mfma(vf[dt], pf, acc_o[dt]);
        if constexpr (NEXT != 2) {
#pragma unroll
          for (int idx = dt * (32 / DT); idx < (dt + 1) * (32 / DT); ++idx) {
            const int mt = idx >> 4, e = idx & 15;
            if (e & 2) mxb = max(mxb, sb[mt][e]); else mxa = max(mxa, sb[mt][e]);
          }
          asm volatile("" : "+v"(mxa), "+v"(mxb));  // keeps this part of the max chain here (integer max re-associates)
        }
        SAGE_FENCE();
      }
#undef SAGE_FENCE
      if constexpr (NEXT != 2) {
        float mx;
        if constexpr (KTHREAD) mx = max_raw((__int_as_float(mxa) - kBiasF) * b0, (__int_as_float(mxb) - kBiasF) * b1);
        else mx = (__int_as_float(max(mxa, mxb)) - kBiasF) * b0;
        mx_cur = swap_max(mx);
      }
    }
    // keep the cross-lane end of the row max (a dependent chain of ~8 instructions with hazard nops) in FRONT of the
    // tile's wait and barrier, where a wave idles anyway: hipcc sank it below the barrier in one of the two unrolled
    // bodies, i.e. in front of the next tile's first MFMA (C3 +1.1 %)
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (SPARSE || PAGED) {  // the window moves on by one list position
      if constexpr (RING == 2) { bw1 = bw2; bw2 = bw_in; }
      else { bw1 = bw2; bw2 = bw3; bw3 = bw4; bw4 = bw_in; }
    }
    if constexpr (RING == 2) {
      dma_wait_all();  // two-slot ring: every copy of this wave has landed before the barrier publishes the tiles
    } else if constexpr (DYN) {
      dma_wait_all();  // the last tiles of a wave drain every copy (the counts of the four-slot ring stay constant)
    } else {
      dma_wait_keep<2 * NDMA>();  // K(j+2), V(j+1) and everything older have landed; the last two iterations' copies fly on
    }
    __syncthreads();
  };
  float nsc0 = 0.f, nsc1 = 0.f;
  int j = 0;
  constexpr std::integral_constant<int, 0> kPlainNext{};
  if constexpr (RING == 4) {
    // four-slot ring: the slot pattern repeats every four tiles
    for (; j + 3 < n_fast; j += 4) {
      fast_iter(std::integral_constant<int, 0>{}, kPlainNext, j, s_cur, s_nxt, sc0, sc1, nsc0, nsc1);
      fast_iter(std::integral_constant<int, 1>{}, kPlainNext, j + 1, s_nxt, s_cur, nsc0, nsc1, sc0, sc1);
      fast_iter(std::integral_constant<int, 2>{}, kPlainNext, j + 2, s_cur, s_nxt, sc0, sc1, nsc0, nsc1);
      fast_iter(std::integral_constant<int, 3>{}, kPlainNext, j + 3, s_nxt, s_cur, nsc0, nsc1, sc0, sc1);
    }
    // up to three fast tiles left (j % 4 == 0 here); after an odd number the live scores sit in the other register set
    bool odd = false;
    if (j < n_fast) {
      fast_iter(std::integral_constant<int, 0>{}, kPlainNext, j, s_cur, s_nxt, sc0, sc1, nsc0, nsc1);
      ++j; odd = true;
      if (j < n_fast) {
        fast_iter(std::integral_constant<int, 1>{}, kPlainNext, j, s_nxt, s_cur, nsc0, nsc1, sc0, sc1);
        ++j; odd = false;
        if (j < n_fast) {
          fast_iter(std::integral_constant<int, 2>{}, kPlainNext, j, s_cur, s_nxt, sc0, sc1, nsc0, nsc1);
          ++j; odd = true;
        }
      }
    }
    if (odd) {
      s_cur[0] = s_nxt[0]; s_cur[1] = s_nxt[1];
      sc0 = nsc0; sc1 = nsc1;
    }
  } else {
  for (; j + 1 < n_fast; j += 2) {
    fast_iter(std::integral_constant<int, 0>{}, kPlainNext, j, s_cur, s_nxt, sc0, sc1, nsc0, nsc1);
    fast_iter(std::integral_constant<int, 1>{}, kPlainNext, j + 1, s_nxt, s_cur, nsc0, nsc1, sc0, sc1);
  }
  // an odd fast tile left (j is even here): one more fast iteration instead of a generic one (+11 % at C2, where the
  // generic body otherwise takes 2 of 32 tiles).
  if (j < n_fast) {
    fast_iter(std::integral_constant<int, 0>{}, kPlainNext, j, s_cur, s_nxt, sc0, sc1, nsc0, nsc1);
    s_cur[0] = s_nxt[0]; s_cur[1] = s_nxt[1];
    sc0 = nsc0; sc1 = nsc1;
    ++j;
  }
  }
  {
    int ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    row_l = q0 + (ln & 31);
    hh_l = ln >> 5;
    if constexpr (CAUSAL && SPLITKV) lim_l = max(row_l / p.q_fold + sk_off, -1);
  }
  // (PAGED: the tail body and the staging-only iterations look their pages up where they need them: a scalar round trip each)
  // staging with run-time slots: the compiler-scheduled tail body below and, for causal waves that are done early, staging-only iterations;
  // every copy drained (vmcnt(0)) -- the four-slot ring keeps its copy COUNT per iteration constant here as well
  auto stage_generic = [&](const int jj) __attribute__((always_inline)) {
    if constexpr (RING == 2) {
      if (jj + 2 < ntiles) dma_k(tile_at(jj + 2), jj & 1, page_at(jj + 2));
      if (jj + 1 < ntiles) load_v(tile_at(jj + 1), (jj + 1) & 1, page_at(jj + 1));
    } else {
      dma_k(ahead(jj + RING), jj % RING, page_at(jj + RING));
      load_v(ahead(jj + RING - 1), (jj + RING - 1) % RING, page_at(jj + RING - 1));
    }
  };
  // The wave's remaining tiles (a successor that may need masking, then its last one).
  //  * FP16 / BF16 PV and FP8 PV at head_dim 64: the same hand-placed stream with
  //    run-time slots (fast_iter, NEXT = 1 / 2): C2 +0.8 %, C2-fp8 +1.6 %, (8,32,2048,128) causal +3.5 %.
  //  * FP8 PV at head_dim 128: the compiler-scheduled body.  With the stream variants instantiated
  //    their MAIN loop came out 0.3-1 % slower (different register assignment), more than the tail tiles return.
  constexpr bool STREAM_TAIL = !(PV_FP8 && D == 128);
  if constexpr (STREAM_TAIL) {
    for (; j + 1 < wave_tiles; ++j) {
      fast_iter(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, j, s_cur, s_nxt, sc0, sc1, nsc0, nsc1);
      s_cur[0] = s_nxt[0]; s_cur[1] = s_nxt[1];
      sc0 = nsc0; sc1 = nsc1;
    }
    if (j < wave_tiles) {
      fast_iter(std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{}, j, s_cur, s_nxt, sc0, sc1, nsc0, nsc1);
      ++j;
    }
  } else {
    for (; j < wave_tiles; ++j) {
      maybe_rescale(mx_cur);
      stage_generic(j);
      const bool has_next = j + 1 < wave_tiles;
      if (has_next) {
        const int jt = tile_at(j + 1);
        tile_scales(jt, nsc0, nsc1, page_at(j + 1));
        qk((j + 1) % RING, s_nxt);
        if (j + 1 >= n_plain) mask_limit(jt, s_nxt);  // a plain last tile (N % 64 == 0, no diagonal) needs none
      }
      if constexpr (PVSKIP) {
        if (pv_skip(j, mx_cur)) ++n_skipped; else softmax_pv(j, j % RING, s_cur, sc0, sc1, std::true_type{});
      } else {
        softmax_pv(j, j % RING, s_cur, sc0, sc1, std::true_type{});
      }
      if (has_next) mx_cur = row_max(s_nxt, nsc0, nsc1);
      dma_wait_all();
      __syncthreads();
      s_cur[0] = s_nxt[0]; s_cur[1] = s_nxt[1];
      sc0 = nsc0; sc1 = nsc1;
    }
  }
  for (; j < ntiles; ++j) {
    stage_generic(j);
    dma_wait_all();
    __syncthreads();
  }

  }

  // ---- epilogue: normalise, (+ v_mean), convert, store; LSE (…sm80.cu:540-668)
  const float l_tot = MROW ? (((row_l - q0) & 16) ? l4[1] : l4[0]) : swap_sum(l_run);
  const float inv = 1.0f / l_tot;
  if constexpr (SPLITKV) {
    // split-KV: the partial result of the split goes to its workspace slot -- the normalised row in fp32, BEFORE any rounding to
    // the output type (rounded, it has the bits the epilogue below stores), and the raw base-2 LSE.  The workspace is dense:
    // a lane's run of 4 channels is one 16-byte store.
    if (row_l < M_) {
      const int64_t srow = ((((int64_t)split * p.B + b) * p.Hq + h) * M_ + row_l);
      float* const wp = p.sk_o + srow * D + 4 * hh_l;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int d0 = 32 * dt + 8 * g4;
          float x[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] = acc_o[dt][4 * g4 + e] * inv;
          if constexpr (PV_FP8) {
            const float4 vs = *reinterpret_cast<const float4*>(p.v_scale + ((int64_t)b * p.Hk + hk) * D + d0 + 4 * hh_l);
            x[0] *= vs.x; x[1] *= vs.y; x[2] *= vs.z; x[3] *= vs.w;
          }
          *reinterpret_cast<float4*>(wp + d0) = make_float4(x[0], x[1], x[2], x[3]);
        }
      if (hh_l == 0) p.sk_lse[srow] = m_run + log2f(l_tot) - kPOff;
    }
  } else if (row_l < M_) {
    uint16_t* op = p.o + o_boff + h * p.osh + (int64_t)row_l * p.osn;
    // A lane holds runs of 4 output channels (8 B); lane ^ 32 holds the neighbouring run of the same row.  The two halves
    // exchange words (v_permlane32_swap) so that each stores 16 contiguous bytes: 8 global_store_dwordx4 per lane instead
    // of 16 dwordx2 (the store tail of a workgroup is bound by the number of store instructions, not by bytes).
    // (instantiated per output element type and store form, selected by ONE uniform branch: as run-time flags inside the
    //  unrolled loops they cost a scalar branch per 4-channel run)
    auto store_rows = [&](auto has_vm, auto obf_tag, auto vec16_tag) __attribute__((always_inline)) {
      constexpr bool OBF = decltype(obf_tag)::value, VEC16 = decltype(vec16_tag)::value;
      const float* vmp = p.v_mean + ((int64_t)b * p.Hk + hk) * D;
      auto run4 = [&](const int dt, const int g4) __attribute__((always_inline)) -> uint2 {
        const int d0 = 32 * dt + 8 * g4 + 4 * hh_l;
        float x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = acc_o[dt][4 * g4 + e] * inv;
        if constexpr (PV_FP8) {  // fuse_v_scale (qk_int_sv_f8_cuda_sm89.cuh:578-626)
          const float4 vs = *reinterpret_cast<const float4*>(p.v_scale + ((int64_t)b * p.Hk + hk) * D + d0);
          x[0] *= vs.x; x[1] *= vs.y; x[2] *= vs.z; x[3] *= vs.w;
        }
        if constexpr (decltype(has_vm)::value) {
          const float4 vmv = *reinterpret_cast<const float4*>(vmp + d0);
          x[0] += vmv.x; x[1] += vmv.y; x[2] += vmv.z; x[3] += vmv.w;
        }
        // o = round16(round32(acc * inv ...)): the fp32 value is made opaque, otherwise hipcc folds the last multiply and the
        // convert into v_fma_mixlo_f16 (one rounding) in SOME instantiations -- more exact by up to one fp16 ulp in ~5e-5 of
        // the elements, but not the arithmetic of the reference epilogue (…sm80.cu:600-640)
#pragma unroll
        for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(x[e]));
        uint2 w;  // packed converts (round to nearest even, as the scalar ones): v_cvt_pk_{f16,bf16}_f32
        if constexpr (OBF) {
          w.x = __builtin_bit_cast(uint32_t, __builtin_convertvector((v2f){x[0], x[1]}, v2bf));
          w.y = __builtin_bit_cast(uint32_t, __builtin_convertvector((v2f){x[2], x[3]}, v2bf));
        } else {
          w.x = __builtin_bit_cast(uint32_t, __builtin_convertvector((v2f){x[0], x[1]}, v2h));
          w.y = __builtin_bit_cast(uint32_t, __builtin_convertvector((v2f){x[2], x[3]}, v2h));
        }
        return w;
      };
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
          // runs A (g4 = 2gp) and B (g4 = 2gp+1): the low half-wave keeps both halves of A, the high one both halves of B
          const uint2 wa = run4(dt, 2 * gp), wb = run4(dt, 2 * gp + 1);
          if constexpr (VEC16) {  // (a row and its lane ^ 32 twin are both inside or both outside the `row < M` guard)
            const auto sx = __builtin_amdgcn_permlane32_swap(wa.x, wb.x, false, false);
            const auto sy = __builtin_amdgcn_permlane32_swap(wa.y, wb.y, false, false);
            *reinterpret_cast<uint4*>(op + 32 * dt + 16 * gp + 8 * hh_l) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
          } else {          // output rows that are only 8-byte aligned: the runs as they are
            *reinterpret_cast<uint2*>(op + 32 * dt + 16 * gp + 4 * hh_l) = wa;
            *reinterpret_cast<uint2*>(op + 32 * dt + 16 * gp + 8 + 4 * hh_l) = wb;
          }
        }
    };
    constexpr std::true_type kT{};
    constexpr std::false_type kF{};
    if (!p.v_mean && p.o_vec16) {  // the common forms
      if (p.out_bf16) store_rows(kF, kT, kT); else store_rows(kF, kF, kT);
    } else if (p.v_mean) {
      if (p.o_vec16) { if (p.out_bf16) store_rows(kT, kT, kT); else store_rows(kT, kF, kT); }
      else { if (p.out_bf16) store_rows(kT, kT, kF); else store_rows(kT, kF, kF); }
    } else {
      if (p.out_bf16) store_rows(kF, kT, kF); else store_rows(kF, kF, kF);
    }
    if (p.lse && hh_l == 0) {
      const float lse2 = m_run + log2f(l_tot) - kPOff;  // base 2, scaled + smoothed logits (…sm80.cu:657-668)
      float* const slot = p.lse + ((int64_t)b * p.Hq + h) * M_ + row_l;
      *slot = p.q_f16 ? lse2 / 1.44269504f + *slot * p.sm_scale : lse2;
    }
  }
  // PVSKIP: the wave's count of skipped tiles, one ordinary store by one lane (a wave without a row < M reports 0)
  if constexpr (PVSKIP) {
    if (p.pv_skipped && row_l == q0 && hh_l == 0)
      p.pv_skipped[((int64_t)bh_row * p.nqb + qb) * 4 + wave] = pv_rows ? n_skipped : 0;
  }
