"""Shared-prefix attention on the paged cache, on the GPU (``sageattn_splitkv_paged_prefix``; the rule:
include/sageattn_hip_prefix.h).

Where one segment alone has keys the check is ``torch.equal`` on bit patterns against the existing operator on that segment;
the general case is held to the bound tests/prefix_util.py derives, against the fp64 merge of what the two existing operators
return for the segments (the prefix one on the folded q, un-folded).

B = 3 suffix sequences and the prefix are the four sequences of ONE cache (``narrow(0, 1)`` / ``narrow(1, B)``), Hq = 4 on
Hk = 2, capacity 512 per table row, 24 pages in a shuffled table (row 2 in descending page order) and a poison page that every
unused entry names.  The caches are prepared at 200 keys per sequence; the calls pass the lengths they test."""
import functools

import pytest
import torch

import paged_util as PU
import prefix_util as XU

pytestmark = pytest.mark.gpu

B, HQ, HK, NCAP, P = 3, 4, 2, 512, 24
FULL = 200
CONFIGS = [(64, 64, "fp8"), (128, 256, "fp16"), (128, 64, "fp8"), (64, 128, "fp16")]   # (D, page_size, pv)
_ID = lambda c: "-".join(str(x) for x in c)  # noqa: E731
SPLITS = [(1, 1), (3, 2), (None, None)]     # (prefix_splits, num_splits)


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    return sageattention_amd


def _lens(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


def _q(M, D, layout="HND", seed=0, dtype=torch.float16):
    g = torch.Generator().manual_seed(31 * D + M + seed)
    q = torch.randn(B, HQ, M, D, generator=g).to(dtype).cuda()
    return q if layout == "HND" else q.transpose(1, 2).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class Setup:
    """pools, one table of B + 1 rows (row 0: the prefix), and the cache of the B + 1 sequences prepared at ``lens_all``;
    ``rows``: a SagePagedRowCache filled from the same rows instead of a SagePagedKVCache bound to the pools"""

    def __init__(self, sa, cfg, lens_all=(FULL,) * (B + 1), lens_max=(FULL,) * (B + 1), layout="HND", rows=False, seed=0,
                 dtype=torch.float16):
        D, ps, pv = cfg
        self.sa, self.cfg, self.layout = sa, cfg, layout
        self.k_pool, self.v_pool, self.poison_page = PU.make_pools(P, HK, ps, D, layout, dtype, "cuda", seed=seed + D + ps)
        self.table_cpu = PU.make_table(list(lens_max), NCAP // ps, ps, P, self.poison_page, seed=seed + 1, reverse_row=2)
        self.table_all = self.table_cpu.cuda()
        self.lens_all = _lens(list(lens_all))
        kw = dict(pv=pv, qk_quant_gran="per_thread", tensor_layout=layout)
        if rows:
            self.whole = sa.SagePagedRowCache.prepare(PU.gather(self.k_pool, self.table_cpu, layout),
                                                      PU.gather(self.v_pool, self.table_cpu, layout), self.table_all,
                                                      self.lens_all, P + 1, ps, **kw)
        else:
            self.whole = sa.SagePagedKVCache.prepare(self.k_pool, self.v_pool, self.table_all, self.lens_all, **kw)
        self.prefix, self.cache = self.whole.narrow(0, 1), self.whole.narrow(1, B)
        self.ptable, self.table = self.table_all[0], self.table_all[1:]

    def run(self, q, Lp, lens, Sp=None, Ss=None, g=1, **kw):
        """(o, lse) of the shared-prefix operator"""
        plen, lens = (Lp if isinstance(Lp, torch.Tensor) else _lens([Lp])), (lens if isinstance(lens, torch.Tensor) else _lens(lens))
        return self.sa.sageattn_splitkv_paged_prefix(q, self.cache, self.table, lens, self.prefix, self.ptable, plen, Ss, Sp,
                                                     q_fold=g, return_lse=True, **kw)

    def segments(self, q, Lp, lens, Sp=None, Ss=None, g=1):
        """what the two EXISTING operators return for the segments: ((o_p, lse_p) un-folded, (o_s, lse_s))"""
        f = self.sa.sageattn_splitkv_paged
        o_p, l_p = f(XU.fold_q(q, self.layout), self.prefix, self.ptable[None], _lens([Lp]), Sp, return_lse=True)
        o_s, l_s = f(q, self.cache, self.table, _lens(lens), Ss, causal=True, q_fold=g, return_lse=True)
        return (XU.unfold_o(o_p, B, self.layout), XU.unfold_lse(l_p, B)), (o_s, l_s)

    def check_general(self, q, Lp, lens, Sp=None, Ss=None, g=1):
        """the operator against the derived bound on the merge of the two segments' results"""
        o, lse = self.run(q, Lp, lens, Sp, Ss, g)
        (o_p, l_p), (o_s, l_s) = self.segments(q, Lp, lens, Sp, Ss, g)
        torch.cuda.synchronize()
        hnd = (lambda t: t) if self.layout == "HND" else (lambda t: t.transpose(1, 2))
        XU.check_prefix(hnd(o), lse, (hnd(o_p), hnd(o_s)), (l_p, l_s), q.dtype)
        return o, lse


@functools.lru_cache(maxsize=None)
def _setup(sa, cfg, layout="HND", rows=False):
    """prepared once at 200 keys per sequence, shared by the tests that only read it"""
    return Setup(sa, cfg, layout=layout, rows=rows)


# ---- 1. one segment alone: the bits of the existing operator; 4. no keys anywhere ------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_degenerate_bits(sa, cfg):
    s = _setup(sa, cfg)
    q = _q(8, cfg[0])
    for Sp, Ss in SPLITS:
        # no prefix: the causal paged operator on the suffixes
        lens = [3, 70, 200]
        o, lse = s.run(q, 0, lens, Sp, Ss, g=2)
        (_, _), (o_s, l_s) = s.segments(q, 0, lens, Sp, Ss, g=2)
        assert torch.equal(_bits(o), _bits(o_s)) and torch.equal(_bits(lse), _bits(l_s)), ("suffix alone", Sp, Ss)
        # no suffix: the non-causal paged operator on the prefix with the folded q, un-folded
        o, lse = s.run(q, FULL, [0, 0, 0], Sp, Ss, g=2)
        (o_p, l_p), (_, _) = s.segments(q, FULL, [0, 0, 0], Sp, Ss, g=2)
        assert torch.equal(_bits(o), _bits(o_p)) and torch.equal(_bits(lse), _bits(l_p)), ("prefix alone", Sp, Ss)
        assert not torch.isnan(o.float()).any() and torch.isfinite(lse).all()
    # mixed: batch 0 has no suffix keys and keeps the prefix bits; the others are held to the bound
    q1 = _q(1, cfg[0])
    lens = [0, 5, 130]
    o, lse = s.check_general(q1, FULL, lens, 3, 2)
    (o_p, l_p), _ = s.segments(q1, FULL, lens, 3, 2)
    assert torch.equal(_bits(o[0]), _bits(o_p[0])) and torch.equal(_bits(lse[0]), _bits(l_p[0]))
    # no keys anywhere: o = 0, lse = -inf
    for Sp, Ss in SPLITS:
        o, lse = s.run(q, 0, [0, 0, 0], Sp, Ss, g=2)
        assert bool((o == 0).all()) and bool(torch.isneginf(lse).all())


# ---- 2. the general case against the derived bound -------------------------------------------------------------------------------
@pytest.mark.parametrize("Lp", [200, 64])
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_general_case(sa, cfg, Lp):
    s = _setup(sa, cfg)
    for Sp, Ss in SPLITS:
        s.check_general(_q(1, cfg[0]), Lp, [1, 70, 130], Sp, Ss)              # a decode step
        s.check_general(_q(8, cfg[0]), Lp, [3, 70, 200], Sp, Ss, g=2)         # four tokens of two rows; batch 0 has 3 keys < 4


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_folded_rows_span_two_q_blocks(sa, cfg):
    """B * M = 144 folded rows are two q-blocks of the prefix pass, the 48 native rows one of the suffix pass"""
    s = _setup(sa, cfg)
    s.check_general(_q(48, cfg[0]), 200, [3, 70, 200], 3, 2, g=2)


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_chunk_longer_than_a_suffix(sa, cfg):
    """T = 8 tokens on suffixes of 3 and 5 keys: the first rows of those batches have no suffix key and see the prefix only"""
    s = _setup(sa, cfg)
    q = _q(8, cfg[0])
    lens = [3, 5, 200]
    o, lse = s.check_general(q, 64, lens, 2, 2)
    (o_p, l_p), (_, l_s) = s.segments(q, 64, lens, 2, 2)
    alone = torch.isneginf(l_s)                                   # [B, HQ, M]: rows without a suffix key
    assert bool(alone[0, :, :5].all()) and bool(alone[1, :, :3].all()) and not bool(alone[2].any())
    assert torch.equal(_bits(o)[alone], _bits(o_p)[alone]) and torch.equal(_bits(lse)[alone], _bits(l_p)[alone])


# ---- 3. poison ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_poison_changes_nothing(sa, cfg):
    """NaN in the rows at or beyond the lengths of the last pages, in every page no table names (state pools included), ids
    beyond the pool in the table entries no sequence needs, NaN in the whole workspace: the bits of the clean call"""
    from sageattention_amd import _lib as L
    from sageattention_amd import prefix as X
    D, ps, pv = cfg
    Lp, lens = 150, [1, 70, 130]
    s = Setup(sa, cfg, lens_all=[Lp] + lens, lens_max=[Lp] + lens)
    q = _q(8, D)
    clean = s.run(q, Lp, lens, 3, 2, g=2)
    c = s.whole
    PU.poison_tails(s.k_pool, s.v_pool, s.table_cpu, [Lp] + lens, "HND")
    need = [PU.pages_needed(n, ps) for n in [Lp] + lens]
    named = {int(p) for b in range(B + 1) for p in s.table_cpu[b, :need[b]]}
    unused = sorted(set(range(P + 1)) - named)
    assert s.poison_page in unused and len(unused) > 1
    for t in (s.k_pool, s.v_pool, c.k_scale):
        t[unused] = float("nan")
    c.k8[unused] = -128
    if c.v8 is not None:
        c.v8.view(torch.uint8)[unused] = 0x7F                   # e4m3 NaN
    for b in range(B + 1):
        s.table_all[b, need[b]:] = P + 1 + b                    # beyond the pool's P + 1 pages
    ws = torch.full((L.lib().sage_prefix_workspace_bytes(B, HQ, 8, D, 3, 2),), 0xFF, dtype=torch.uint8, device="cuda")
    assert torch.isnan(ws.view(torch.float32)).all()
    fp8 = pv == "fp8"
    got = X._prefix_attn(q, c.k8, c.k_scale, s.cache.km, c.v8 if fp8 else s.v_pool, s.cache.v_scale if fp8 else None, s.table,
                         _lens(lens), s.ptable, _lens([Lp]), s.prefix.km, s.prefix.v_scale if fp8 else None, 2, 3, 2, "HND",
                         D ** -0.5, "per_thread", True, workspace=ws)
    again = s.run(q, Lp, lens, 3, 2, g=2)
    torch.cuda.synchronize()
    for o, lse in (got, again):
        assert torch.equal(_bits(o), _bits(clean[0])) and torch.equal(_bits(lse), _bits(clean[1]))
        assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any()


# ---- 5. HIP graph --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(128, 256, "fp16"), (64, 64, "fp8")], ids=_ID)
def test_graph_replay(sa, cfg):
    """{append; shared-prefix attention} captured once; then both tables are permuted in place with the pages moved
    accordingly and prefix_len and kv_lens grow: the replay equals an eager call on the new state"""
    lens0, lens1 = [64, 1, 70, 130], [200, 3, 70, 200]
    s = Setup(sa, cfg, lens_all=lens0, lens_max=lens1)
    c = s.whole
    q = _q(8, cfg[0])
    start, lens = _lens(lens0), s.lens_all
    attn = lambda: sa.sageattn_splitkv_paged_prefix(q, s.cache, s.table, lens[1:], s.prefix, s.ptable, lens[:1], 2, 3,  # noqa: E731
                                                    q_fold=2, return_lse=True)
    step = lambda: (c.append(s.table_all, start, lens, 136), attn())[1]  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up (start = len: the ragged tiles again, the same bits)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og, lg = step()
    g = torch.Generator().manual_seed(9)
    perm = torch.cat([torch.randperm(P, generator=g), torch.tensor([P])])
    inv = torch.argsort(perm).cuda()
    for t in [s.k_pool, s.v_pool, c.k8, c.k_scale] + ([c.v8.view(torch.uint8)] if c.v8 is not None else []):
        t.copy_(t[inv])
    s.table_all.copy_(perm[s.table_cpu.long()].to(torch.int32).cuda())
    lens.copy_(_lens(lens1))
    og.fill_(1.0); lg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    oe, le = attn()                                               # eager, on the state the replay's append left
    torch.cuda.synchronize()
    assert torch.equal(_bits(og), _bits(oe)) and torch.equal(_bits(lg), _bits(le))
    assert not torch.isnan(og.float()).any() and torch.isfinite(lg).all()
    # ... and that state is the one a fresh cache reaches by the same append: the general bound on its segments
    XU.check_prefix(og, lg, *zip(*s.segments(q, lens1[0], lens1[1:], 3, 2, g=2)), q.dtype)


# ---- 6. torch.compile ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_compile_fullgraph(sa, pv):
    """one step {append; shared-prefix attention} under torch.compile(fullgraph=True) gives the eager bits"""
    cfg = (128, 64, pv)
    lens0, lens1 = [64, 1, 70, 130], [66, 3, 70, 134]
    s, e = (Setup(sa, cfg, lens_all=lens0, lens_max=[FULL] * 4) for _ in range(2))
    q = _q(4, cfg[0])

    def step(x, table_all, qq, start, lens):
        x.whole.append(table_all, start, lens, 4)
        return sa.sageattn_splitkv_paged_prefix(qq, x.cache, table_all[1:], lens[1:], x.prefix, table_all[0], lens[:1], 2, 3,
                                                q_fold=2, return_lse=True)

    torch.compiler.reset()
    fn = torch.compile(lambda table_all, qq, start, lens: step(s, table_all, qq, start, lens), backend="aot_eager", fullgraph=True)
    oc, lc = fn(s.table_all, q, _lens(lens0), _lens(lens1))
    oe, le = step(e, e.table_all, q, _lens(lens0), _lens(lens1))
    torch.cuda.synchronize()
    assert torch.equal(_bits(oc), _bits(oe)) and torch.equal(_bits(lc), _bits(le))
    assert not torch.isnan(oc.float()).any() and torch.isfinite(lc).all()


# ---- 7. both cache classes; NHD pools with a strided q ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(64, 64, "fp8"), (128, 256, "fp16")], ids=_ID)
def test_both_cache_classes(sa, cfg):
    """a SagePagedRowCache and a SagePagedKVCache built from the same rows give identical bits"""
    bound, rows = _setup(sa, cfg), _setup(sa, cfg, rows=True)
    assert isinstance(rows.whole, sa.SagePagedRowCache) and isinstance(bound.whole, sa.SagePagedKVCache)
    for M, g, lens in ((1, 1, [1, 70, 130]), (8, 2, [3, 70, 200])):
        q = _q(M, cfg[0])
        a, b = bound.run(q, 200, lens, 3, 2, g=g), rows.run(q, 200, lens, 3, 2, g=g)
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.parametrize("cfg", [(128, 64, "fp8"), (64, 128, "fp16")], ids=_ID)
def test_nhd_pools_and_a_strided_q(sa, cfg):
    """q as a view into a wider projection output: sliced along heads and channels its folded view keeps one row stride and
    it is read in place; sliced along the rows as well it travels as one copy.  The bits of the contiguous q either way"""
    s = _setup(sa, cfg, layout="NHD")
    D, M = cfg[0], 8
    want = None
    for rows in (M, 2 * M):
        big = torch.full((B, rows, HQ + 1, 2 * D), float("nan"), dtype=torch.float16, device="cuda")
        q = big[:, rows - M:, :HQ, D:]
        q.copy_(_q(M, D, layout="NHD"))
        assert not q.is_contiguous()
        o, lse = s.check_general(q, 200, [3, 70, 200], 3, 2, g=2)
        assert o.shape == q.shape and o.is_contiguous()
        want = want or s.run(q.contiguous(), 200, [3, 70, 200], 3, 2, g=2)
        assert torch.equal(o, want[0]) and torch.equal(lse, want[1])


def test_bf16(sa):
    """bf16 q, pools and output: the merge's other rounding"""
    cfg = (64, 64, "fp8")
    s = Setup(sa, cfg, dtype=torch.bfloat16)
    q = _q(8, cfg[0], dtype=torch.bfloat16)
    o, lse = s.check_general(q, 200, [3, 70, 200], 3, 2, g=2)
    assert o.dtype == torch.bfloat16
    o, lse = s.run(q, 0, [3, 70, 200], 3, 2, g=2)
    _, (o_s, l_s) = s.segments(q, 0, [3, 70, 200], 3, 2, g=2)
    assert torch.equal(_bits(o), _bits(o_s)) and torch.equal(_bits(lse), _bits(l_s))
