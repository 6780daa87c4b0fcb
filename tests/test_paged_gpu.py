"""The paged KV cache on the GPU (``SagePagedKVCache``, ``sageattn_splitkv_paged``; the rule: include/sageattn_hip_paged.h).

Paging is an addressing change, so every check is ``torch.equal`` on bit patterns against code that exists without it: the
reference is ``SageKVCache`` / ``sageattn_splitkv_cached`` on the padded tensors gathered from the pages (tests/paged_util.py),
taken through the same appends.  No tolerance anywhere.

B = 3, Hq = 4 on Hk = 2, capacity N = 512, lengths [0, 65, 300] growing to [0, 130, 512], 24 pages and a poison page (NaN rows)
that every unused table entry names; tables are a random draw, row 2 in descending page order."""
import functools

import pytest
import torch

import kvcache_util as KU
import paged_util as PU

pytestmark = pytest.mark.gpu

B, HQ, HK, N, P = 3, 4, 2, 512, 24
LENS0, LENS1 = [0, 65, 300], [0, 130, 512]
# (D, page_size, pv, gran): per-thread scales everywhere, page size 256 once, per-block K scales ("per_warp") once
CONFIGS = [(D, ps, pv, "per_thread") for D in (64, 128) for ps in (64, 128) for pv in ("fp16", "fp8")]
CONFIGS += [(128, 256, "fp8", "per_thread"), (64, 128, "fp8", "per_warp")]
_ID = lambda c: "-".join(str(x) for x in c)  # noqa: E731
FILL = 0xA5


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    return sageattention_amd


def _lens(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


def _q(M, D, dtype=torch.float16, seed=0, layout="HND"):
    g = torch.Generator().manual_seed(31 * D + M + seed)
    q = torch.randn(B, HQ, M, D, generator=g).to(dtype).cuda()
    return q if layout == "HND" else q.transpose(1, 2).contiguous()


class Setup:
    """pools, a table for ``lens_max``, the paged cache prepared at ``lens`` and the contiguous reference on the gathered
    tensors (gathered from the CLEAN pools: the reference never sees a NaN tail)"""

    def __init__(self, sa, cfg, lens, lens_max, layout="HND", dtype=torch.float16, poison_tails=False, seed=0):
        D, ps, pv, gran = cfg
        self.sa, self.cfg, self.layout, self.poison = sa, cfg, layout, poison_tails
        self.k_pool, self.v_pool, self.poison_page = PU.make_pools(P, HK, ps, D, layout, dtype, "cuda", seed=seed + D + ps)
        self.clean_k, self.clean_v = self.k_pool.clone(), self.v_pool.clone()
        self.table_cpu = PU.make_table(lens_max, N // ps, ps, P, self.poison_page, seed=seed + 1, reverse_row=2)
        self.table = self.table_cpu.cuda()
        self.set_rows(lens)
        kw = dict(pv=pv, qk_quant_gran=gran, tensor_layout=layout)
        self.ref = sa.SageKVCache.prepare(PU.gather(self.clean_k, self.table_cpu, layout),
                                          PU.gather(self.clean_v, self.table_cpu, layout), _lens(lens), **kw)
        self.cache = sa.SagePagedKVCache.prepare(self.k_pool, self.v_pool, self.table, _lens(lens), **kw)
        self.lens = list(lens)

    def set_rows(self, lens):
        """the pools as the caller would have them at these lengths: with ``poison_tails`` the rows >= len_b of each
        sequence's last page are NaN"""
        if self.poison:
            self.k_pool.copy_(self.clean_k)
            self.v_pool.copy_(self.clean_v)
            PU.poison_tails(self.k_pool, self.v_pool, self.table_cpu, lens, self.layout)

    def append(self, start, lens, max_new):
        self.set_rows(lens)
        self.cache.append(self.table, _lens(start), _lens(lens), max_new)
        self.ref.append(_lens(start), _lens(lens), max_new)
        self.lens = list(lens)

    def check_state(self):
        PU.assert_state_equals_ref(self.cache, self.ref, self.table_cpu, self.lens)

    def attention(self, q, **kw):
        """(o, lse) of the paged operator and of the contiguous one on the reference, after checking them equal bit for bit,
        free of NaN, and o = 0 / lse = -inf for the batch without keys"""
        lens = _lens(self.lens)
        o, lse = self.sa.sageattn_splitkv_paged(q, self.cache, self.table, lens, return_lse=True, **kw)
        ro, rlse = self.sa.sageattn_splitkv_cached(q, self.ref, lens, return_lse=True, **kw)
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), ro.view(torch.int16)), ("o", kw)
        assert torch.equal(lse.view(torch.int32), rlse.view(torch.int32)), ("lse", kw)
        assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any()
        for b, n in enumerate(self.lens):
            if n == 0:
                ob = o[b]
                assert bool((ob == 0).all()) and bool((lse[b] == float("-inf")).all())
        return o, lse


# the chain of appends of the state test: (start lens, lens, max_new)
CHAIN = [([0, 65, 300], [0, 66, 301], 1),       # one row; max_new smaller than any page
         ([0, 66, 301], [0, 63, 301], 1),       # a rollback (start >= len), and start == len: the ragged tile again
         ([0, 63, 301], [0, 65, 301], 2),       # 63 -> 65 across a tile
         ([0, 65, 301], [0, 130, 390], 100),    # across the page boundaries 128 (row 1) and 320 / 384 (row 2)
         ([0, 130, 390], [0, 130, 512], 122)]   # to the end of the capacity (across 448 and, for 256-key pages, into the last)


# ---- 1. state ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_state_after_prepare_and_appends(sa, cfg):
    """after ``prepare`` and after every append of the chain each valid tile equals the reference's, bit for bit, the frozen
    statistics are the reference's, and every byte of the state pools outside the touched tiles still holds the fill"""
    s = Setup(sa, cfg, LENS0, LENS1)
    s.check_state()
    c = s.cache
    pools = [c.k8, c.k_scale] + ([c.v8] if c.v8 is not None else [])
    for t in pools:
        t.view(torch.uint8).fill_(FILL)
    c.prepare_(s.table, _lens(LENS0))           # the same statistics again, and every valid page by one append from 0
    s.check_state()
    spans = [([0, 0, 0], LENS0)]
    for start, lens, max_new in CHAIN:
        s.append(start, lens, max_new)
        s.check_state()
        spans.append((start, lens))
    mk, ms, mv = PU.touched_masks(c, s.table_cpu, spans)
    layout = c.tensor_layout
    k8 = PU.hnd_pool(c.k8, layout).view(torch.uint8).cpu()
    assert bool((k8[~mk] == FILL).all()), "k8 outside the touched tiles"
    assert bool((c.k_scale.view(torch.uint8).cpu().view(*c.k_scale.shape, 4)[~ms] == FILL).all()), "k_scale outside"
    if mv is not None:
        assert bool((PU.hnd_pool(c.v8, layout).view(torch.uint8).cpu()[~mv] == FILL).all()), "v8 outside the touched blocks"
    # the poison page and every page no sequence names: untouched, whatever the masks say
    unused = sorted(set(range(P + 1)) - {int(p) for b in range(B) for p in s.table_cpu[b, :PU.pages_needed(LENS1[b], c.page_size)]})
    assert s.poison_page in unused and bool((k8[unused] == FILL).all())


@functools.lru_cache(maxsize=None)
def _grown(sa, cfg, layout="HND"):
    """prepared at LENS0 and appended to LENS1 in one call (shared by the attention tests; nothing changes it)"""
    s = Setup(sa, cfg, LENS0, LENS1, layout=layout)
    s.append(LENS0, LENS1, 212)
    s.check_state()
    return s


# ---- 2. attention --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_splits", [1, 3, None])
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_attention_non_causal(sa, cfg, num_splits):
    s = _grown(sa, cfg)
    s.attention(_q(70, cfg[0]), num_splits=num_splits)


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_attention_causal(sa, cfg, num_splits):
    s = _grown(sa, cfg)
    s.attention(_q(16, cfg[0]), num_splits=num_splits, causal=True, q_fold=4)


def test_attention_at_the_prepared_lengths(sa):
    """... and before any append: ragged last tiles in the middle of a page, a table whose later entries name real pages"""
    for cfg in [(64, 64, "fp8", "per_thread"), (128, 128, "fp16", "per_thread")]:
        s = Setup(sa, cfg, LENS0, LENS1)
        s.attention(_q(70, cfg[0]), num_splits=3)
        s.attention(_q(16, cfg[0]), num_splits=2, causal=True, q_fold=4)


# ---- 3. poison -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_poison_changes_nothing(sa, cfg):
    """the poison page behind the last valid entry of every row and NaN in the rows >= len_b of every last page: the bits of
    the clean run -- the reference is built from the clean pools -- and no NaN"""
    s = Setup(sa, cfg, LENS0, LENS0, poison_tails=True)        # the table ends at ceil(len_b / page_size) entries
    for b, n in enumerate(LENS0):
        assert bool((s.table_cpu[b, PU.pages_needed(n, cfg[1]):] == s.poison_page).all())
    assert torch.isnan(s.k_pool[:P].float()).any() and torch.isnan(s.v_pool[:P].float()).any()
    s.check_state()
    for ns in (1, 3, None):
        s.attention(_q(70, cfg[0]), num_splits=ns)
    for ns in (1, 3):
        s.attention(_q(16, cfg[0]), num_splits=ns, causal=True, q_fold=4)
    s.append(LENS0, [0, 66, 301], 1)                            # one more row: the tail behind it is NaN again
    s.check_state()
    s.attention(_q(70, cfg[0]), num_splits=3)
    s.attention(_q(16, cfg[0]), num_splits=1, causal=True, q_fold=4)


# ---- 4. NHD pools, q a strided view ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(64, 64, "fp8", "per_thread"), (128, 128, "fp16", "per_thread"), (64, 128, "fp16", "per_thread"),
                                 (128, 64, "fp8", "per_thread")], ids=_ID)
def test_nhd_pools_and_a_strided_q(sa, cfg):
    s = _grown(sa, cfg, "NHD")
    D = cfg[0]
    for M, kw in ((70, dict(num_splits=3)), (16, dict(num_splits=2, causal=True, q_fold=4))):
        big = torch.full((B, 2 * M, HQ + 1, 2 * D), float("nan"), dtype=torch.float16, device="cuda")
        q = big[:, M:, :HQ, D:]
        q.copy_(_q(M, D, layout="NHD"))
        assert not q.is_contiguous()
        o, lse = s.attention(q, **kw)
        o2, lse2 = s.attention(q.contiguous(), **kw)
        assert torch.equal(o, o2) and torch.equal(lse, lse2) and o.shape == q.shape and o.is_contiguous()


# ---- 5. HIP graph --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(128, 128, "fp16", "per_thread"), (64, 64, "fp8", "per_thread")], ids=_ID)
def test_graph_replay(sa, cfg):
    """{append; attention} captured once; then the lengths change AND the table is permuted with the pages moved accordingly,
    all in place: the replay equals an eager call on the new state and the reference"""
    s = Setup(sa, cfg, LENS0, LENS1)
    c = s.cache
    q = _q(16, cfg[0])
    start, lens = _lens(LENS0), _lens(LENS0)
    step = lambda: (c.append(s.table, start, lens, 212),  # noqa: E731
                    sa.sageattn_splitkv_paged(q, c, s.table, lens, 3, causal=True, q_fold=4, return_lse=True))[1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up (start = len: the ragged tiles again, the same bits)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og, lg = step()
    # move every page: page p goes to perm[p] in all pools (the poison page stays), and the table follows
    g = torch.Generator().manual_seed(9)
    perm = torch.cat([torch.randperm(P, generator=g), torch.tensor([P])])
    inv = torch.argsort(perm).cuda()
    for t in [s.k_pool, s.v_pool, s.clean_k, s.clean_v, c.k8, c.k_scale] + ([c.v8.view(torch.uint8)] if c.v8 is not None else []):
        t.copy_(t[inv])
    s.table_cpu = perm[s.table_cpu.long()].to(torch.int32)
    s.table.copy_(s.table_cpu.cuda())
    s.check_state()                                           # the moved state is the reference's still
    start.copy_(_lens(LENS0)); lens.copy_(_lens(LENS1))
    og.fill_(1.0); lg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    s.ref.append(_lens(LENS0), _lens(LENS1), 212)
    s.lens = list(LENS1)
    s.check_state()
    oe, le = s.attention(q, num_splits=3, causal=True, q_fold=4)      # eager, on the new state; equal to the reference's
    assert torch.equal(og, oe) and torch.equal(lg, le)


# ---- 6. torch.compile ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_compile_fullgraph(sa, pv):
    """one decode step {append; attention} under torch.compile(fullgraph=True) gives the eager bits"""
    cfg = (128, 128, pv, "per_thread")
    s, e = Setup(sa, cfg, LENS0, LENS1), Setup(sa, cfg, LENS0, LENS1)
    q = _q(4, cfg[0])

    def step(c, table, qq, start, lens):
        c.append(table, start, lens, 4)
        return sa.sageattn_splitkv_paged(qq, c, table, lens, 3, return_lse=True)

    torch.compiler.reset()
    fn = torch.compile(lambda table, qq, start, lens: step(s.cache, table, qq, start, lens), backend="aot_eager", fullgraph=True)
    new = [0, 66, 301]
    oc, lc = fn(s.table, q, _lens(LENS0), _lens(new))
    oe, le = step(e.cache, e.table, q, _lens(LENS0), _lens(new))
    torch.cuda.synchronize()
    assert torch.equal(oc, oe) and torch.equal(lc, le)
    s.ref.append(_lens(LENS0), _lens(new), 4)
    s.lens = new
    s.check_state()
    ro, rl = s.attention(q, num_splits=3)
    assert torch.equal(oc, ro) and torch.equal(lc, rl)


# ---- 7. narrow + prepare_ --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(64, 64, "fp8", "per_thread"), (128, 128, "fp16", "per_thread")], ids=_ID)
def test_narrow_prepares_one_slot(sa, cfg):
    """slot 1 gets a new sequence in new pages: ``narrow(1, 1).prepare_`` writes its statistics and its pages, and every page
    of the other slots -- and their statistics -- keep their bytes"""
    s = Setup(sa, cfg, LENS0, LENS1)
    c, ps = s.cache, cfg[1]
    used = {int(p) for b in range(B) for p in s.table_cpu[b, :PU.pages_needed(LENS1[b], ps)]}
    free = sorted(set(range(P)) - used)
    new_len = 100
    need = PU.pages_needed(new_len, ps)
    row = torch.full((1, N // ps), s.poison_page, dtype=torch.int32)
    row[0, :need] = torch.tensor(free[:need][::-1], dtype=torch.int32)
    state = [c.k8, c.k_scale, c.km] + ([c.v8.view(torch.uint8), c.v_scale, c.v_coef] if c.v8 is not None else [])
    before = [t.clone() for t in state]
    c.narrow(1, 1).prepare_(row.cuda(), _lens([new_len]))
    torch.cuda.synchronize()
    mine = torch.tensor(free[:need])
    for t, old in zip(state[:2] + state[3:4], before[:2] + before[3:4]):       # the pools: only the new pages changed
        keep = torch.ones(P + 1, dtype=torch.bool)
        keep[mine] = False
        assert torch.equal(t[keep.cuda()], old[keep.cuda()])
        assert not torch.equal(t[mine.cuda()], old[mine.cuda()])
    for t, old in zip([state[2]] + state[4:], [before[2]] + before[4:]):       # per-sequence statistics: only slot 1
        assert torch.equal(t[0], old[0]) and torch.equal(t[2], old[2]) and not torch.equal(t[1], old[1])
    # the whole cache against a reference with that sequence in slot 1
    s.table_cpu[1] = row[0]
    s.table.copy_(s.table_cpu.cuda())
    lens = [LENS0[0], new_len, LENS0[2]]
    kw = dict(pv=cfg[2], qk_quant_gran=cfg[3])
    s.ref = sa.SageKVCache.prepare(PU.gather(s.clean_k, s.table_cpu, "HND"), PU.gather(s.clean_v, s.table_cpu, "HND"), _lens(lens), **kw)
    s.lens = lens
    s.check_state()
    s.attention(_q(16, cfg[0]), num_splits=2, causal=True, q_fold=4)


# ---- 8. far pages ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_far_pages(sa, pv):
    """HND pools of 131072 + 8 pages of 64 keys at head_dim 128, 4 GiB and eight pages each, allocated and not filled; one
    sequence in the pages {0, 65537, P-1, 1, P-2}: byte offsets beyond 2^31 in the INT8 and FP8 pools and beyond 2^32 in the
    fp16 pools"""
    D, ps, Pf = 128, 64, 131072 + 8
    need_gib = 12
    free = torch.cuda.mem_get_info()[0] / 2 ** 30
    if free < 16:
        pytest.skip(f"needs about {need_gib} GiB of device memory with 16 GiB free, {free:.1f} GiB are free")
    pages = [0, 65537, Pf - 1, 1, Pf - 2]
    k_pool = torch.empty((Pf, HK, ps, D), dtype=torch.float16, device="cuda")
    v_pool = torch.empty_like(k_pool)
    g = torch.Generator().manual_seed(77)
    for p in pages:
        k_pool[p] = (torch.randn(HK, ps, D, generator=g) + 0.4).half().cuda()
        v_pool[p] = torch.randn(HK, ps, D, generator=g).half().cuda()
    assert k_pool[Pf - 1].data_ptr() - k_pool.data_ptr() > 2 ** 32 and (Pf - 1) * HK * ps * D > 2 ** 31
    table_cpu = torch.tensor([pages], dtype=torch.int32)
    table = table_cpu.cuda()
    lens0, lens1 = [200], [300]
    kw = dict(pv=pv, qk_quant_gran="per_thread")
    gk = torch.stack([k_pool[p] for p in pages]).permute(1, 0, 2, 3).reshape(1, HK, 5 * ps, D).contiguous()
    gv = torch.stack([v_pool[p] for p in pages]).permute(1, 0, 2, 3).reshape(1, HK, 5 * ps, D).contiguous()
    ref = sa.SageKVCache.prepare(gk, gv, _lens(lens0), **kw)
    cache = sa.SagePagedKVCache.prepare(k_pool, v_pool, table, _lens(lens0), **kw)
    PU.assert_state_equals_ref(cache, ref, table_cpu, lens0)
    cache.append(table, _lens(lens0), _lens(lens1), 100)
    ref.append(_lens(lens0), _lens(lens1), 100)
    PU.assert_state_equals_ref(cache, ref, table_cpu, lens1)
    lens = _lens(lens1)
    gq = torch.Generator().manual_seed(5)
    for M, kws in ((70, dict(num_splits=1)), (70, dict(num_splits=3)), (70, dict()), (16, dict(num_splits=2, causal=True, q_fold=4))):
        q = torch.randn(1, HQ, M, D, generator=gq).half().cuda()
        o, lse = sa.sageattn_splitkv_paged(q, cache, table, lens, return_lse=True, **kws)
        ro, rlse = sa.sageattn_splitkv_cached(q, ref, lens, return_lse=True, **kws)
        torch.cuda.synchronize()
        assert torch.equal(o, ro) and torch.equal(lse, rlse), kws
        assert not torch.isnan(o.float()).any()
