"""Decode attention on the paged MXFP4 V cache, one wave per split (``sageattn_decode_paged_v4``,
include/sageattn_hip_decode_fp4.h), on the GPU: the bits of ``sageattn_splitkv_paged_v4(causal=True)``, a plain float64 softmax,
poison behind the lengths, one HIP graph and torch.compile."""
import functools
import itertools

import pytest
import torch

import paged_util as PU
import splitkv_causal_util as CU

pytestmark = pytest.mark.gpu

HK, CAP = 2, 512                              # 8 tiles: the K ring wraps, S = 16 has empty splits, S = 3 uneven ones
LENS = (0, 1, 2, 63, 64, 65, 200, 512)       # length 2 with T = 3 and T = 4: rows without keys
FOLDS = ((1, 1), (1, 4), (3, 4), (4, 8))     # (T, g)
GRID = list(itertools.product((64, 128), ("per_thread", "per_warp"), (64, 256)))  # page 64: every tile is a new page


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    return sageattention_amd


@functools.lru_cache(maxsize=None)
def _setup(D, gran, page_size):
    """-> (cache, table, lens, spare): random pools behind a permuted table whose unused entries name ``spare``, a valid page
    no sequence owns"""
    import sageattention_amd as sa
    k, v, P = PU.make_pools(24, HK, page_size, D, "HND", torch.float16, "cuda", seed=D + page_size)
    spare = P - 1
    table = PU.make_table(LENS, CAP // page_size, page_size, P - 1, spare, seed=5, reverse_row=7).cuda()
    lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    return sa.SagePagedKVCacheV4.prepare(k, v, table, lens, qk_quant_gran=gran), table, lens, spare


def _rand_q(T, g, D):
    """q [B, T, HK * g, D] and its folded view [B, HK, T * g, D]"""
    q = torch.randn(len(LENS), T, HK * g, D, generator=torch.Generator().manual_seed(11)).to(torch.float16).cuda()
    return q, q.reshape(len(LENS), T, HK, g, D).permute(0, 2, 1, 3, 4).reshape(len(LENS), HK, T * g, D)


def _same(a, b):
    return all(torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32),
                           y.view(torch.int16 if y.element_size() == 2 else torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("D,gran,page_size", GRID, ids=str)
def test_bits_of_the_causal_paged_operator(sa, D, gran, page_size):
    cache, table, lens, _ = _setup(D, gran, page_size)
    for (T, g), S in itertools.product(FOLDS, (1, 3, 8, 16)):
        _, qf = _rand_q(T, g, D)
        got = sa.sageattn_decode_paged_v4(qf, cache, table, lens, num_splits=S, q_fold=g, return_lse=True)
        want = sa.sageattn_splitkv_paged_v4(qf, cache, table, lens, num_splits=S, causal=True, q_fold=g, return_lse=True)
        assert _same(got, want), (T, g, S)


def _float64_rule(cache, table, q):
    """softmax in float64 over the 16-bit K / V rows gathered from the pages, keys 0 <= j <= t + len_b - T; no operator of the
    library.  q [B, T, Hq, D] -> o [B, T, Hq, D], lse [B, T, Hq] (a row without keys: o = 0, lse = -inf)"""
    kg, vg = PU.gather(cache.k, table, "HND").double(), PU.gather(cache.v, table, "HND").double()
    B, T, Hq, D = q.shape
    o = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    lse = torch.full(q.shape[:3], float("-inf"), dtype=torch.float64, device=q.device)
    for b, n in enumerate(LENS):
        if n:
            kk, vv = (x[b, :, :n].repeat_interleave(Hq // HK, dim=0) for x in (kg, vg))
            s = q[b].double().transpose(0, 1) @ kk.transpose(1, 2) * D ** -0.5
            s = s.masked_fill(~CU.allowed_keys(n, T, 1).to(q.device), float("-inf"))
            l = torch.logsumexp(s, dim=-1)
            p = torch.exp(s - torch.where(torch.isneginf(l), torch.zeros_like(l), l).unsqueeze(-1))
            o[b], lse[b] = (p @ vv).transpose(0, 1), l.transpose(0, 1)
    return o, lse


def _errors(o, lse, g, o64, l64):
    """max |o - o64| and max |lse - lse64| of a folded result; rows without keys exactly 0 and -inf"""
    B, T, Hq, D = o64.shape
    o = o.reshape(B, HK, T, g, D).transpose(1, 2).reshape(B, T, Hq, D)
    lse = lse.reshape(B, HK, T, g).transpose(1, 2).reshape(B, T, Hq)
    none = torch.isneginf(l64)
    assert bool(torch.isneginf(lse[none]).all()) and bool((o[none] == 0).all()) and bool(torch.isfinite(lse[~none]).all())
    return float((o.double() - o64).abs().max()), float((lse.double()[~none] - l64[~none]).abs().max())


@pytest.mark.parametrize("D,gran,page_size", GRID, ids=str)
def test_against_float64_softmax(sa, D, gran, page_size):
    """The yardstick is the existing operator's own error against float64 on the same inputs, measured in this run; the margin
    1.25 is that of test_decode_gpu.py and reads 1.0 while the bits are equal."""
    cache, table, lens, _ = _setup(D, gran, page_size)
    for T, g in FOLDS:
        q, qf = _rand_q(T, g, D)
        ref = _float64_rule(cache, table, q)
        kw = dict(num_splits=3, q_fold=g, return_lse=True)
        yo, yl = _errors(*sa.sageattn_splitkv_paged_v4(qf, cache, table, lens, causal=True, **kw), g, *ref)
        eo, el = _errors(*sa.sageattn_decode_paged_v4(qf, cache, table, lens, **kw), g, *ref)
        print(f"D={D} {gran} page={page_size} T={T} g={g}: o {eo:.4e} / {yo:.4e}, lse {el:.4e} / {yl:.4e}")
        assert eo <= 1.25 * yo and el <= 1.25 * yl


@pytest.mark.parametrize("D", [64, 128])
def test_poison_behind_the_lengths_changes_no_bit(sa, D):
    """clean run, then the spare page every unused table entry names overwritten in every pool and 127 into the INT8 rows at or
    beyond len_b of every last page; the image columns behind len_b keep the zeros the append wrote (the cache's invariant)"""
    cache, table, lens, spare = _setup.__wrapped__(D, "per_thread", 256)
    _, qf = _rand_q(3, 4, D)
    clean = sa.sageattn_decode_paged_v4(qf, cache, table, lens, num_splits=3, q_fold=4, return_lse=True)
    cache.v4[spare] = 0xFF
    cache.v4_scale[spare] = 0xFF
    cache.k8[spare] = 127
    cache.k_scale[spare] = float("nan")
    for b, n in enumerate(LENS):
        if n % 256:
            cache.k8[int(table[b, (n - 1) // 256]), :, n % 256:] = 127
    got = sa.sageattn_decode_paged_v4(qf, cache, table, lens, num_splits=3, q_fold=4, return_lse=True)
    assert _same(got, clean) and bool(torch.isfinite(got[0]).all())


def test_append_and_attention_in_one_graph(sa):
    """{append; decode attention} captured once; then the lengths are changed in place and two sequences trade their pages, and
    every replay equals the eager call on the new values"""
    cache, table, lens, _ = _setup.__wrapped__(128, "per_thread", 64)
    _, qf = _rand_q(1, 4, 128)

    def step():
        cache.append(table, lens, lens, 1)
        return sa.sageattn_decode_paged_v4(qf, cache, table, lens, num_splits=3, q_fold=4, return_lse=True)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og, lg = step()
    lens.copy_(torch.tensor([3, 0, 60, 64, 1, 200, 65, 100], dtype=torch.int32).cuda())
    table[[5, 7]] = table[[7, 5]]                                              # sequences 5 and 7 trade their pages
    oe, le = step()
    for _ in range(3):
        og.fill_(1.0); lg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same((og, lg), (oe, le))


def test_compile_fullgraph(sa):
    cache, table, lens, _ = _setup(64, "per_thread", 64)
    _, qf = _rand_q(3, 4, 64)
    torch.compiler.reset()
    got = torch.compile(lambda qq, tab, ln: sa.sageattn_decode_paged_v4_compilable(qq, cache, tab, ln, 3, 4, return_lse=True),
                        backend="aot_eager", fullgraph=True)(qf, table, lens)
    torch.cuda.synchronize()
    assert _same(got, sa.sageattn_decode_paged_v4(qf, cache, table, lens, num_splits=3, q_fold=4, return_lse=True))
