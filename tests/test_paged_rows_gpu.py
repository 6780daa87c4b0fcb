"""The paged cache without fp16 pools on the GPU (``SagePagedRowCache``; the rule: include/sageattn_hip_paged_rows.h).

Nothing numerical is new, so every check is ``torch.equal`` on bit patterns.  The reference is ``SagePagedKVCache`` over fp16 /
bf16 pools into which the same rows were written (tests/paged_rows_util.py ``scatter_rows``), with the same block table, lengths,
granularity and ``v_headroom``, taken through the same calls.  No tolerance anywhere.

B = 3, Hq = 4 on Hk = 2, capacity 512 keys, a permuted table with spare pages.  Poison: the ring starts as NaN, the rows of
``k_new`` / ``v_new`` at or beyond n_b are NaN, the reference's pools start as NaN, and the state pools start as a byte pattern
that every byte outside the touched tiles and the named pages must keep (a snapshot before every call)."""
import functools

import pytest
import torch

import paged_rows_util as RU
import paged_util as PU

pytestmark = pytest.mark.gpu

B, HQ, HK, N = 3, 4, 2, RU.CAP
SPARE = 3
FILL = 0xA5
# (D, page_size, pv, gran, dtype, layout, strided rows): head_dim 64 and 128 with pages of 64 and 256 (128 once), both P.V
# forms, per_thread and per_warp, bf16 once, NHD once, k_new / v_new a strided view of a fused projection once
F16, BF16 = torch.float16, torch.bfloat16
CONFIGS = [(64, 64, "fp16", "per_thread", F16, "HND", False), (64, 256, "fp8", "per_thread", F16, "HND", False),
           (128, 64, "fp8", "per_thread", F16, "HND", False), (128, 256, "fp16", "per_thread", F16, "HND", False),
           (64, 64, "fp8", "per_warp", F16, "HND", False), (128, 128, "fp16", "per_warp", F16, "HND", False),
           (128, 64, "fp8", "per_thread", BF16, "HND", False), (64, 256, "fp16", "per_thread", F16, "NHD", False),
           (64, 128, "fp8", "per_thread", F16, "NHD", False), (128, 256, "fp8", "per_thread", F16, "HND", True)]
_ID = lambda c: "-".join(str(x).replace("torch.", "") for x in c[:6]) + ("-strided" if c[6] else "")  # noqa: E731


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    return sageattention_amd


def _lens(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


def _q(M, D, dtype, layout, seed=0):
    g = torch.Generator().manual_seed(31 * D + M + seed)
    q = torch.randn(B, HQ, M, D, generator=g).to(dtype).cuda()
    return q if layout == "HND" else q.transpose(1, 2).contiguous()


class Setup:
    """the cache under test and the reference, prepared from one padded prompt at ``lens`` and taken through the same calls"""

    def __init__(self, sa, cfg, lens, seed=0):
        D, ps, pv, gran, dtype, layout, strided = cfg
        self.sa, self.cfg, self.D, self.ps, self.dtype, self.layout, self.strided = sa, cfg, D, ps, dtype, layout, strided
        self.gen = torch.Generator().manual_seed(1000 * seed + D + ps)
        self.P = B * (N // ps) + SPARE
        self.table_cpu = PU.make_table([N] * B, N // ps, ps, self.P, self.P - 1, seed=seed + 1, reverse_row=2)
        self.table = self.table_cpu.cuda()
        self.named = sorted({int(p) for p in self.table_cpu.flatten()})
        assert len(self.named) == B * (N // ps) and len(set(range(self.P)) - set(self.named)) == SPARE
        # the reference's pools: NaN wherever no row was written
        shape = (self.P, HK, ps, D) if layout == "HND" else (self.P, ps, HK, D)
        self.k_pool = torch.full(shape, float("nan"), dtype=dtype, device="cuda")
        self.v_pool = torch.full(shape, float("nan"), dtype=dtype, device="cuda")
        kw = dict(pv=pv, qk_quant_gran=gran, tensor_layout=layout)
        self.cache = sa.SagePagedRowCache.allocate(self.P, ps, B, HK, D, dtype, "cuda", **kw)
        for t in (self.cache.k8, self.cache.k_scale, self.cache.v):
            t.view(torch.uint8).fill_(FILL)
        self.cache.k_tail.fill_(float("nan"))
        N0 = max(max(lens), 1)
        k, v = self.rows(N0, [0] * B, lens)
        self.prefix_vmax = float(torch.nan_to_num(v.float(), nan=0.0).abs().max())
        zeros = [0] * B
        RU.scatter_rows(self.k_pool, self.table_cpu, layout, zeros, lens, self.hnd(k))
        RU.scatter_rows(self.v_pool, self.table_cpu, layout, zeros, lens, self.hnd(v))
        self.ref = sa.SagePagedKVCache.prepare(self.k_pool, self.v_pool, self.table, _lens(lens), **kw)
        before = RU.state_bytes(self.cache)
        self.cache.prepare_(k, v, self.table, _lens(lens))
        if pv == "fp8":   # a sequence without keys has no V statistics (the pre-pass writes none): give both caches the same
            for c in (self.cache, self.ref):
                for b, n in enumerate(lens):
                    if n == 0:
                        c.v_scale[b], c.v_coef[b, :, 0], c.v_coef[b, :, 1] = 1.0, 0.0, 1.0
        self.lens = list(lens)
        self.check(before, zeros, lens, k)

    def hnd(self, rows):
        return rows if self.layout == "HND" else rows.transpose(1, 2)

    def rows(self, T, starts, lens, v_mult=None):
        """k_new, v_new of a call in the cache's layout: random rows, NaN at and beyond n_b; ``strided``: views into a fused
        [B, T, 3, Hk, D] projection output whose other third is NaN"""
        k = (torch.randn(B, HK, T, self.D, generator=self.gen) * 1.5 + 0.3).to(self.dtype).cuda()
        v = torch.randn(B, HK, T, self.D, generator=self.gen).to(self.dtype).cuda()
        if v_mult is not None:
            v = (v.float() * (v_mult / float(v.float().abs().max()))).to(self.dtype)
        for b, (s, n) in enumerate(zip(starts, lens)):
            k[b, :, max(n - s, 0):] = float("nan")
            v[b, :, max(n - s, 0):] = float("nan")
        if self.strided:
            assert self.layout == "HND"
            fused = torch.full((B, T, 3, HK, self.D), float("nan"), dtype=self.dtype, device="cuda")
            fused[:, :, 1], fused[:, :, 2] = k.transpose(1, 2), v.transpose(1, 2)
            k, v = fused[:, :, 1].transpose(1, 2), fused[:, :, 2].transpose(1, 2)
            assert not k.is_contiguous() and k.stride(-1) == 1
            return k, v
        return (k, v) if self.layout == "HND" else (k.transpose(1, 2).contiguous(), v.transpose(1, 2).contiguous())

    def call(self, starts, lens, T, v_mult=None):
        k, v = self.rows(T, starts, lens, v_mult)
        RU.scatter_rows(self.k_pool, self.table_cpu, self.layout, starts, lens, self.hnd(k))
        RU.scatter_rows(self.v_pool, self.table_cpu, self.layout, starts, lens, self.hnd(v))
        self.ref.append(self.table, _lens(starts), _lens(lens), T)
        before = RU.state_bytes(self.cache)
        self.cache.append_rows(k, v, self.table, _lens(starts), _lens(lens))
        self.lens = list(lens)
        self.check(before, starts, lens, k)

    def check(self, before, starts, lens, k_new):
        """every valid tile and the statistics equal the reference's; nothing outside what the call may write has changed;
        the ring holds the input rows of [s_b, len_b) within the last two tiles"""
        torch.cuda.synchronize()
        c = self.cache
        RU.assert_state_equals_ref(c, self.ref, self.table_cpu, lens)
        masks = RU.write_masks(c, self.table_cpu, starts, lens)
        after = RU.state_bytes(c)
        for name, m, a, b0 in zip(("k8", "k_scale", "v", "k_tail"), masks, after, before):
            assert torch.equal(a[~m], b0[~m]), f"{name}: bytes outside what the call may write"
        spare = sorted(set(range(self.P)) - set(self.named))
        for a in after[:3]:
            assert bool((a[spare] == FILL).all()), "a page no sequence names"
        kh = self.hnd(k_new)
        for b, (s, n) in enumerate(zip(starts, lens)):
            rows = list(RU.ring_written_rows(s, n, N))
            if rows:
                r = torch.tensor(rows)
                got = c.k_tail[b, :, ((r >> 6) & 1).cuda(), (r & 63).cuda()]
                want = kh[b][:, (r - RU.call_geometry(s, n, N)[0]).cuda()]
                assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16)), ("ring", b)

    def attention(self, q, **kw):
        lens = _lens(self.lens)
        o, lse = self.sa.sageattn_splitkv_paged(q, self.cache, self.table, lens, return_lse=True, **kw)
        ro, rlse = self.sa.sageattn_splitkv_paged(q, self.ref, self.table, lens, return_lse=True, **kw)
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), ro.view(torch.int16)), ("o", kw)
        assert torch.equal(lse.view(torch.int32), rlse.view(torch.int32)), ("lse", kw)
        assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any()
        return o, lse


LENS0 = [0, 63, 130]


def _decode_chain(s):
    """the calls of the first chain, from the lengths [0, 63, 130]"""
    fp8 = s.cfg[2] == "fp8"
    for step in range(3):                                            # three T = 1 steps: batch 1 across 63 -> 66
        s.call([0, 63 + step, 130 + step], [0, 64 + step, 131 + step], 1)
    # T = 4 with n_b = [4, 0, 2]: the middle batch re-quantizes its ragged tile from the ring.  FP8: the new V rows reach 3x
    # the prefix maximum, beyond the frozen range of v_headroom = 2, and saturate as the reference's do
    s.call([0, 66, 133], [4, 66, 135], 4, v_mult=3 * s.prefix_vmax if fp8 else None)
    if fp8:
        v8 = PU.hnd_pool(s.ref.v8, s.layout).view(torch.uint8)
        assert bool(((v8[s.named] & 0x7F) == 0x7E).any()), "no V byte of the reference saturated at 448"
    s.call([4, 66, 135], [4, 63, 135], 1)                            # rollback 66 -> 63 (s = len = 63) ...
    s.call([4, 63, 135], [4, 65, 135], 2)                            # ... then an append of 2
    s.call([4, 65, 135], [5, 66, 136], 1)
    s.call([5, 62, 136], [5, 67, 136], 5)                            # overwrite and extend: s = 62, len = 67 at old length 66
    s.call([5, 67, 136], [205, 267, 336], 200)                       # T = 200
    s.call([205, 300, 336], [205, 267, 400], 64)                     # start >= len beside a chunk of a whole tile
    s.call([205, 267, 400], [206, 268, 512], 112)                    # to the end of the capacity


# ---- 1. state ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_state_after_prepare_and_calls(sa, cfg):
    s = Setup(sa, cfg, LENS0)
    _decode_chain(s)


@pytest.mark.parametrize("cfg", CONFIGS[:4] + CONFIGS[6:7], ids=_ID)
def test_a_chunk_across_two_tile_boundaries(sa, cfg):
    """T = 70 from 60 to 130: the last tile has the parity of the first, so the ring rows read for tile 0 are the rows written
    for tile 2 (batch 2: tiles 1 and 3).  Then the ring serves a decode step and the ragged tile again"""
    s = Setup(sa, cfg, [0, 60, 124], seed=1)
    s.call([0, 60, 124], [0, 130, 194], 70)
    s.call([0, 130, 194], [0, 131, 195], 1)
    s.call([0, 131, 195], [0, 131, 195], 1)
    s.call([0, 131, 195], [0, 100, 256], 61)                         # a rollback across one tile boundary beside a chunk
    s.call([0, 100, 256], [0, 129, 257], 29)


def test_prepare_again_on_a_narrowed_cache(sa):
    """``narrow`` shares the pools: preparing sequence 1 again leaves the others' state and ring alone"""
    cfg = CONFIGS[2]
    s = Setup(sa, cfg, LENS0)
    c1, r1 = s.cache.narrow(1, 1), s.ref.narrow(1, 1)
    k, v = s.rows(200, [0] * B, [0, 200, 0])
    RU.scatter_rows(s.k_pool, s.table_cpu, s.layout, [0] * B, [0, 200, 0], k)
    RU.scatter_rows(s.v_pool, s.table_cpu, s.layout, [0] * B, [0, 200, 0], v)
    r1.prepare_(s.table[1:2], _lens([200]))
    before = RU.state_bytes(s.cache)
    c1.prepare_(k[1:2], v[1:2], s.table[1:2], _lens([200]))
    s.check(before, [0, 0, 130], [0, 200, 130], k)


# ---- 2. attention --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grown(sa, cfg):
    s = Setup(sa, cfg, LENS0)
    s.call(LENS0, [0, 66, 301], 171)
    return s


@pytest.mark.parametrize("cfg", CONFIGS[:4] + CONFIGS[6:9], ids=_ID)
def test_attention_equals_the_reference(sa, cfg):
    s = _grown(sa, cfg)
    D, dtype, layout = cfg[0], cfg[4], cfg[5]
    for ns in (1, 3):
        s.attention(_q(70, D, dtype, layout), num_splits=ns)
        s.attention(_q(16, D, dtype, layout), num_splits=ns, causal=True, q_fold=2)


# ---- 3. one HIP graph, torch.compile ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [CONFIGS[1], CONFIGS[3]], ids=_ID)
def test_step_in_one_hip_graph(sa, cfg):
    """{append_rows; attention} captured once and replayed after lengths, table and k_new changed in place"""
    s = Setup(sa, cfg, LENS0)
    D, dtype, layout = cfg[0], cfg[4], cfg[5]
    q = _q(4, D, dtype, layout)
    starts, lens, table = _lens(LENS0), _lens([0, 64, 131]), s.table.clone()
    k, v = s.rows(1, LENS0, [0, 64, 131])
    k, v = k.clone(), v.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture, on the state the first replay will see again
        snapshot = [t.clone() for t in (s.cache.k8, s.cache.k_scale, s.cache.v, s.cache.k_tail)]
        s.cache.append_rows(k, v, table, starts, lens)
        sa.sageattn_splitkv_paged(q, s.cache, table, lens, 2, causal=True, q_fold=2, return_lse=True)
        for t, old in zip((s.cache.k8, s.cache.k_scale, s.cache.v, s.cache.k_tail), snapshot):
            t.copy_(old)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.cache.append_rows(k, v, table, starts, lens)
        o, lse = sa.sageattn_splitkv_paged(q, s.cache, table, lens, 2, causal=True, q_fold=2, return_lse=True)
    cur = list(LENS0)
    for new in ([0, 64, 131], [0, 65, 132]):
        k2, v2 = s.rows(1, cur, new)
        k.copy_(k2), v.copy_(v2), starts.copy_(_lens(cur)), lens.copy_(_lens(new))
        if new[1] == 65:   # the table changes in place too: sequences 1 and 2 swap the pages of their unused last entries
            last = table.size(1) - 1
            table[1, last], table[2, last] = s.table[2, last], s.table[1, last]
        graph.replay()
        RU.scatter_rows(s.k_pool, s.table_cpu, layout, cur, new, s.hnd(k))
        RU.scatter_rows(s.v_pool, s.table_cpu, layout, cur, new, s.hnd(v))
        s.ref.append(s.table, _lens(cur), _lens(new), 1)
        ro, rlse = sa.sageattn_splitkv_paged(q, s.ref, s.table, _lens(new), 2, causal=True, q_fold=2, return_lse=True)
        torch.cuda.synchronize()
        RU.assert_state_equals_ref(s.cache, s.ref, s.table_cpu, new)
        assert torch.equal(o.view(torch.int16), ro.view(torch.int16)) and torch.equal(lse.view(torch.int32), rlse.view(torch.int32))
        cur = new


def test_step_under_torch_compile(sa):
    cfg = CONFIGS[2]
    s = Setup(sa, cfg, LENS0)
    q = _q(4, cfg[0], cfg[4], cfg[5])
    new = [0, 64, 131]
    k, v = s.rows(1, LENS0, new)

    def step(q, k, v, table, starts, lens):
        s.cache.append_rows(k, v, table, starts, lens)
        return sa.sageattn_splitkv_paged(q, s.cache, table, lens, 2, return_lse=True)

    torch.compiler.reset()
    o, lse = torch.compile(step, backend="aot_eager", fullgraph=True)(q, k, v, s.table, _lens(LENS0), _lens(new))
    RU.scatter_rows(s.k_pool, s.table_cpu, s.layout, LENS0, new, k)
    RU.scatter_rows(s.v_pool, s.table_cpu, s.layout, LENS0, new, v)
    s.ref.append(s.table, _lens(LENS0), _lens(new), 1)
    ro, rlse = sa.sageattn_splitkv_paged(q, s.ref, s.table, _lens(new), 2, return_lse=True)
    torch.cuda.synchronize()
    RU.assert_state_equals_ref(s.cache, s.ref, s.table_cpu, new)
    assert torch.equal(o.view(torch.int16), ro.view(torch.int16)) and torch.equal(lse.view(torch.int32), rlse.view(torch.int32))
