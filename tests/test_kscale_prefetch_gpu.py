"""The K scales the attention tile loop dequantises a tile with are those of THAT tile, whatever the tile count.

The loop requests the scales of tile j+2 (and, block-sparse / paged, the list entry or page that enters its window) at the end
of iteration j, and its fast loops are unrolled by the ring (2 or 4 slots); what can go wrong is an index: a tile computed with
the scales of a neighbour, at the prologue, at an unroll remainder, at the hand-over to the wave's last tiles or at the clamp
behind the last tile.  So the key counts stand around those boundaries -- 1, 2, 3, 4, 5 and 9 tiles, and 200 keys whose last
tile is masked -- and every 64-key tile has its own magnitude, 2^(t mod 5): the quantizer gives neighbouring tiles scales a
factor of 2 (behind tile 4: 16) apart.  K carries a component along one direction u that q sees with a random sign per row, so
that for some rows the small tiles hold the mass and for others the large ones: whichever tile takes a neighbour's scales, rows
exist whose result moves (test_oracle_separates_the_tiles checks that on the CPU, by swapping scales in the oracle).

M = 256, B = 1, Hq = 2 on Hk = 1 (GQA), head_dim 64 and 128, per-warp and per-thread scales, FP16 / BF16 / FP8 P.V, causal and
not, in both geometries (4 and 8 waves).  Reference: oracle/sage_oracle.py; tolerances: those of the operators' end-to-end tests
against the same oracle (tests/test_gpu_parity.py, tests/test_block_sparse_gpu.py)."""
import pytest
import torch

B, HQ, HK, M = 1, 2, 1, 256
NS = (64, 128, 192, 200, 256, 320, 576)
# max |o - oracle|: FP16 PV fp16 / bf16 outputs, FP8 PV (test_gpu_parity.test_end_to_end_vs_oracle, test_block_sparse_gpu._TOL)
TOL = {"fp16": 2e-3, "bf16": 1.6e-2, "fp8": 0.06}
LSE_TOL = 3e-3


def make_qkv(N, D, pv, seed=0):
    """q, k, v (HND, CPU) in the input dtype of the mode.  Rows of key tile t: 2^(t mod 5) * (0.35 noise + u), u = 1/sqrt(D) in
    every channel; q: noise + 2.5 a * sqrt(D) * u with a ~ N(0, 1) per row, so a key of tile t gets a logit offset of about
    2^(t mod 5) * 2.5 a / sqrt(D): rows with a < 0 favour the small tiles, rows with a > 0 the large ones."""
    g = torch.Generator().manual_seed(100 * N + D + seed)
    dt = torch.bfloat16 if pv == "bf16" else torch.float16
    nt = (N + 63) // 64
    mag = (2.0 ** (torch.arange(nt) % 5)).repeat_interleave(64)[:N].view(1, 1, N, 1)
    u = torch.full((D,), D ** -0.5)
    k = mag * (0.35 * torch.randn(B, HK, N, D, generator=g) + u)
    a = torch.randn(B, HQ, M, 1, generator=g)
    q = torch.randn(B, HQ, M, D, generator=g) + 2.5 * a * (D ** 0.5) * u
    # V within +-0.5, the sign by tile: mass that moves between neighbouring tiles moves o by up to 0.8 of it, while one e4m3
    # step (2^-4) of even a weight-one key moves o by at most 2^-4 * |v - o| <= 0.0625 -- the FP8 tolerance is made for that
    sign = (1.0 - 2.0 * (torch.arange(nt) % 2)).repeat_interleave(64)[:N].view(1, 1, N, 1)
    v = 0.4 * sign + (0.1 * torch.randn(B, HK, N, D, generator=g)).clamp(-0.1, 0.1)
    return q.to(dt), k.to(dt), v.to(dt)


def oracle(q, k, v, pv, gran, causal, swap=None, attn_mask=None):
    """sageattn_oracle spelled out so that the K scales (and an element mask) can be reached: -> (o, lse).
    swap = (t0, t1): the scale groups of these two key tiles exchanged -- what a loop that mixes tiles up computes."""
    from oracle import sage_oracle as O
    D = q.shape[-1]
    sm_scale = D ** -0.5
    km = O.k_mean(k, "HND")
    quant = O.per_thread_int8 if gran == "per_thread" else O.per_warp_int8
    q8, qs, k8, ks = quant(q, k, km, tensor_layout="HND")
    if swap is not None:
        per = ks.shape[-1] // ((k.shape[2] + 63) // 64)
        ks = ks.clone()
        t0, t1 = swap
        a, b = ks[..., t0 * per:(t0 + 1) * per].clone(), ks[..., t1 * per:(t1 + 1) * per].clone()
        ks[..., t0 * per:(t0 + 1) * per], ks[..., t1 * per:(t1 + 1) * per] = b, a
    qrows, kcols = O.expand_q_scale(qs, q.shape[2], gran), O.expand_k_scale(ks, k.shape[2], gran)
    mult = sm_scale * 1.4426950408889634
    if pv == "fp8":
        v8, v_scale, _ = O.per_channel_fp8(v, tensor_layout="HND", smooth_v=False)
        o, lse2 = O.attn_tile_loop(q8, k8, v8, qrows, kcols, logit_mult=mult, is_causal=causal, pv="fp8", v_scale=v_scale,
                                   out_dtype=q.dtype, attn_mask=attn_mask)
    else:
        o, lse2 = O.attn_tile_loop(q8, k8, v, qrows, kcols, logit_mult=mult, is_causal=causal, out_dtype=q.dtype,
                                   attn_mask=attn_mask)
    return o, lse2 / 1.4426950408889634 + O.lse_correction(q, km, "HND") * sm_scale


@pytest.mark.parametrize("pv", ["fp16", "bf16", "fp8"])
@pytest.mark.parametrize("gran", ["per_warp", "per_thread"])
@pytest.mark.parametrize("D", [64, 128])
def test_oracle_separates_the_tiles(D, gran, pv):
    """CPU: on these inputs the oracle with the scales of two neighbouring tiles exchanged -- every neighbouring pair of
    every key count -- is far from the oracle: at least 10 tolerances of the 16-bit modes (0.02 / 0.16) and 3 of FP8 PV (0.18: V
    lies within +-0.5, so no result can move by more than 1, and the FP8 tolerance is 0.06).  (N = 64 has one tile.)"""
    for N in NS[1:]:
        q, k, v = make_qkv(N, D, pv)
        o, _ = oracle(q, k, v, pv, gran, False)
        for t in range((N + 63) // 64 - 1):
            o_sw, _ = oracle(q, k, v, pv, gran, False, swap=(t, t + 1))
            moved = (o_sw.float() - o.float()).abs().max().item()
            print(f"N {N} D {D} {gran} {pv}: tiles {t}/{t + 1} swapped -> max |do| {moved:.3f}")
            assert moved > (3 if pv == "fp8" else 10) * TOL[pv], (N, t, moved)


@pytest.fixture(scope="module")
def sa():
    assert torch.cuda.is_available()
    import sageattention_amd
    return sageattention_amd


def _pinned(nw):
    from constructed_gpu_util import _pinned as pin
    return pin(nw)


def _check(o, lse, oo, ol, pv, what):
    do = (o.cpu().float() - oo.float()).abs().max().item()
    fin = torch.isfinite(ol)
    dl = (lse.cpu() - ol)[fin].abs().max().item()
    print(f"{what}: max |do| {do:.3e}  max |dlse| {dl:.3e}")
    assert torch.isfinite(o).all()
    assert do < TOL[pv], (what, do)
    assert dl < LSE_TOL, (what, dl)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("pv", ["fp16", "bf16", "fp8"])
@pytest.mark.parametrize("gran", ["per_warp", "per_thread"])
@pytest.mark.parametrize("D", [64, 128])
def test_dense_every_tile_count(sa, D, gran, pv, causal):
    """The dense operators at every key count of NS, 4 and 8 waves, against the oracle; and the two geometries against each
    other bit for bit: they are on the parent for every one of these cases (the same arithmetic per 32-row wave)."""
    op = sa.sageattn_qk_int8_pv_fp8_cuda if pv == "fp8" else sa.sageattn_qk_int8_pv_fp16_cuda
    for N in NS:
        q, k, v = make_qkv(N, D, pv)
        oo, ol = oracle(q, k, v, pv, gran, causal)
        got = {}
        for nw in (4, 8):
            with _pinned(nw):
                o, lse = op(q.cuda(), k.cuda(), v.cuda(), is_causal=causal, qk_quant_gran=gran, return_lse=True)
                torch.cuda.synchronize()
            _check(o, lse, oo, ol, pv, f"dense N {N} D {D} {gran} {pv} causal {causal} nw {nw}")
            got[nw] = (o.cpu(), lse.cpu())
        assert torch.equal(got[4][0], got[8][0]) and torch.equal(got[4][1], got[8][1]), N


@pytest.mark.gpu
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_kv_lens(sa, D, pv):
    """sageattn_kvlen: 576 keys of which 200 / 320 count -- the oracle on the first len keys (the operator's own rule)."""
    N = 576
    for n in (200, 320):
        q, k, v = make_qkv(N, D, pv, seed=n)
        lens = torch.tensor([n], dtype=torch.int32, device="cuda")
        for nw in (4, 8):
            with _pinned(nw):
                o, lse = sa.sageattn_kvlen(q.cuda(), k.cuda(), v.cuda(), lens, pv=pv, return_lse=True)
                torch.cuda.synchronize()
            oo, ol = oracle(q, k[:, :, :n], v[:, :, :n], pv, "per_thread", False)
            _check(o, lse, oo, ol, pv, f"kv_lens {n}/{N} D {D} {pv} nw {nw}")


@pytest.mark.gpu
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_split_kv(sa, D, pv):
    """sageattn_splitkv, 9 tiles over 2 and 4 splits (5 + 4; 3 + 3 + 3): every split's loop starts at its own first tile.
    The merged result is the dense one up to the fp32 merge: the dense tolerance."""
    N = 576
    q, k, v = make_qkv(N, D, pv, seed=3)
    oo, ol = oracle(q, k, v, pv, "per_thread", False)
    for S in (2, 4):
        o, lse = sa.sageattn_splitkv(q.cuda(), k.cuda(), v.cuda(), num_splits=S, pv=pv, return_lse=True)
        torch.cuda.synchronize()
        _check(o, lse, oo, ol, pv, f"split-KV S {S} D {D} {pv}")


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_paged_split_kv(sa, D, causal):
    """sageattn_splitkv_paged, page size 64, the 9 pages of the sequence scattered over a pool of 12 in descending order with
    gaps: the page of a tile differs from its position.  FP16 PV; 1 and 2 splits.  causal: aligned to the end of the keys, the
    M = 256 rows are the last 256 positions -- the oracle's top-left mask on the key axis shifted by N - M."""
    N, P = 576, 12
    q, k, v = make_qkv(N, D, "fp16", seed=5)
    pages = [11, 9, 8, 6, 5, 4, 2, 1, 0]
    k_pool = torch.zeros(P, HK, 64, D, dtype=torch.float16)
    v_pool = torch.zeros(P, HK, 64, D, dtype=torch.float16)
    for t, pg in enumerate(pages):
        k_pool[pg], v_pool[pg] = k[0, :, 64 * t:64 * t + 64], v[0, :, 64 * t:64 * t + 64]
    table = torch.tensor([pages], dtype=torch.int32, device="cuda")
    lens = torch.tensor([N], dtype=torch.int32, device="cuda")
    cache = sa.SagePagedKVCache.prepare(k_pool.cuda(), v_pool.cuda(), table, lens, pv="fp16")
    mask = None
    if causal:
        mask = (torch.arange(N).view(1, 1, 1, N) <= torch.arange(M).view(1, 1, M, 1) + (N - M)).expand(B, HQ, M, N)
    oo, ol = oracle(q, k, v, "fp16", "per_thread", False, attn_mask=mask)
    for S in (1, 2):
        o, lse = sa.sageattn_splitkv_paged(q.cuda(), cache, table, lens, num_splits=S, causal=causal, return_lse=True)
        torch.cuda.synchronize()
        _check(o, lse, oo, ol, "fp16", f"paged split-KV S {S} D {D} causal {causal}")


@pytest.mark.gpu
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_block_sparse_with_gaps(sa, D, pv):
    """sageattn_block_sparse on 9 key tiles with a map that has gaps (q-block 0: tiles 0 2 3 5 8, q-block 1: 1 4 6 7 8 and,
    second head, 3 alone): the tile at a list position is not the position.  Oracle: the tile loop under the expanded map."""
    from blocksparse_util import expand_map
    N = 576
    q, k, v = make_qkv(N, D, pv, seed=7)
    bm = torch.zeros(B, HQ, 2, 9, dtype=torch.bool)
    bm[0, 0, 0, [0, 2, 3, 5, 8]] = True
    bm[0, 0, 1, [1, 4, 6, 7, 8]] = True
    bm[0, 1, 0, [1, 2, 3, 4, 5, 6, 7]] = True
    bm[0, 1, 1, 3] = True
    oo, ol = oracle(q, k, v, pv, "per_thread", False, attn_mask=expand_map(bm, M, N))
    for nw in (4, 8):
        with _pinned(nw):
            o, lse = sa.sageattn_block_sparse(q.cuda(), k.cuda(), v.cuda(), bm.cuda(), pv=pv, return_lse=True)
            torch.cuda.synchronize()
        _check(o, lse, oo, ol, pv, f"block-sparse D {D} {pv} nw {nw}")
