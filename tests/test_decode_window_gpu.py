"""Decode attention with a sliding window and sink logits (``sageattn_decode_paged_window``,
include/sageattn_hip_decode_window.h) on the GPU: the bits of ``sageattn_splitkv_paged_window`` on both launch paths, pages that
left the window and rows behind the lengths, a plain float64 softmax, one HIP graph and torch.compile.  Geometry, pools and
queries are those of test_decode_gpu.py."""
import itertools

import pytest
import torch

import paged_util as PU
import splitkv_causal_util as CU
from test_decode_gpu import FOLDS, GRID, HK, KINDS, LENS, _errors, _rand_q, _same, _setup

pytestmark = pytest.mark.gpu

WINDOWS = (1, 2, 63, 64, 65, 100, 129, 512, 10000)   # one key, both sides of a tile edge, a start inside tile 1, >= capacity


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    return sageattention_amd


def _sinks(g):
    s = torch.randn(HK * g, generator=torch.Generator().manual_seed(3)) * 2
    s[0], s[-1] = 30.0, -30.0
    return s.cuda()


@pytest.mark.parametrize("D,kind,gran,page_size", GRID, ids=str)
def test_bits_of_the_four_wave_window_operator(sa, D, kind, gran, page_size):
    """S = 1 is the one-launch path, S = 3 and 16 leave empty splits"""
    cache, table, lens, _ = _setup(D, *kind, gran, page_size)
    for (T, g), S, window in itertools.product(FOLDS, (1, 2, 3, 16), WINDOWS):
        _, qf = _rand_q(T, g, D, kind[1])
        for sinks in (None, _sinks(g)):
            kw = dict(num_splits=S, q_fold=g, sinks=sinks, return_lse=True)
            got = sa.sageattn_decode_paged_window(qf, cache, table, lens, window, **kw)
            assert _same(got, sa.sageattn_splitkv_paged_window(qf, cache, table, lens, window, **kw)), (T, g, S, window, sinks)
        if window == 10000:                                                    # no window, no sinks: the decode operator
            kw = dict(num_splits=S, q_fold=g)
            got = sa.sageattn_decode_paged_window(qf, cache, table, lens, window, return_lse=True, **kw)
            assert _same(got, sa.sageattn_decode_paged(qf, cache, table, lens, return_lse=True, **kw)), (T, g, S)
            assert torch.equal(got[0], sa.sageattn_decode_paged_window(qf, cache, table, lens, window, **kw))  # (no lse asked)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("D,kind", list(itertools.product((64, 128), KINDS)), ids=str)
def test_the_window_is_exactly_the_window(sa, D, kind, S):
    """clean run; then the table entries of the pages that left the window name the spare page, which is overwritten in every
    pool, and the rows at or beyond len_b of every last page are poisoned as in test_decode_gpu.py"""
    pv, dtype = kind
    cache, table, lens, spare = _setup.__wrapped__(D, pv, dtype, "per_thread", 64)
    _, qf = _rand_q(3, 4, D, dtype)
    kw = dict(num_splits=S, q_fold=4, sinks=_sinks(4), return_lse=True)
    clean = sa.sageattn_decode_paged_window(qf, cache, table, lens, 100, **kw)
    freed = table.clone()
    for b, n in enumerate(LENS):
        freed[b, :max(n - 3 - 100 + 1, 0) // 64] = spare
    assert int((freed != table).sum()) >= 7
    PU.poison_tails(cache.k, cache.v, table, LENS, "HND")
    for b, n in enumerate(LENS):
        if n % 64:
            cache.k8[int(table[b, (n - 1) // 64]), :, n % 64:] = 127
    cache.k[spare] = cache.v[spare] = cache.k_scale[spare] = float("nan")
    cache.k8[spare] = 127
    if pv == "fp8":
        cache.v8.view(torch.uint8)[spare] = 0x7f
    got = sa.sageattn_decode_paged_window(qf, cache, freed, lens, 100, **kw)
    assert _same(got, clean) and bool(torch.isfinite(got[0]).all())


def _float64_rule(cache, table, q, window, sinks):
    """softmax in float64 over the 16-bit K / V rows gathered from the pages, keys max(0, t + off - window + 1) <= j <= t + off,
    the sink in the denominator; no operator of the library.  q [B, T, Hq, D] -> o [B, T, Hq, D], lse [B, T, Hq] (a row
    without keys: o = 0, lse = -inf)"""
    kg, vg = PU.gather(cache.k, table, "HND").double(), PU.gather(cache.v, table, "HND").double()
    B, T, Hq, D = q.shape
    o = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    lse = torch.full(q.shape[:3], float("-inf"), dtype=torch.float64, device=q.device)
    for b, n in enumerate(LENS):
        if n:
            kk, vv = (x[b, :, :n].repeat_interleave(Hq // HK, dim=0) for x in (kg, vg))
            s = q[b].double().transpose(0, 1) @ kk.transpose(1, 2) * D ** -0.5
            first = torch.arange(T).view(-1, 1) + CU.off_of(n, T, 1) - window + 1
            allowed = CU.allowed_keys(n, T, 1) & (torch.arange(n).view(1, -1) >= first)
            s = s.masked_fill(~allowed.to(q.device), float("-inf"))
            keys = torch.logsumexp(s, dim=-1)                                  # [Hq, T]
            l = torch.where(torch.isneginf(keys), keys, torch.logaddexp(keys, sinks.double().view(-1, 1)))
            p = torch.exp(s - torch.where(torch.isneginf(l), torch.zeros_like(l), l).unsqueeze(-1))
            o[b], lse[b] = (p @ vv).transpose(0, 1), l.transpose(0, 1)
    return o, lse


@pytest.mark.parametrize("window", [100, 129])
@pytest.mark.parametrize("D,kind,gran,page_size", GRID, ids=str)
def test_against_float64_softmax(sa, D, kind, gran, page_size, window):
    """The yardstick is the four-wave operator's own error against float64 on the same inputs, measured in this run; the
    margin 1.25 is that of test_decode_gpu.py and reads 1.0 while the bits are equal."""
    cache, table, lens, _ = _setup(D, *kind, gran, page_size)
    for (T, g), S in itertools.product(FOLDS, (1, 3)):
        q, qf = _rand_q(T, g, D, kind[1])
        ref = _float64_rule(cache, table, q, window, _sinks(g))
        kw = dict(num_splits=S, q_fold=g, sinks=_sinks(g), return_lse=True)
        yo, yl = _errors(*sa.sageattn_splitkv_paged_window(qf, cache, table, lens, window, **kw), g, *ref)
        eo, el = _errors(*sa.sageattn_decode_paged_window(qf, cache, table, lens, window, **kw), g, *ref)
        print(f"D={D} {kind} {gran} page={page_size} T={T} g={g} S={S} window={window}: o {eo:.4e} / {yo:.4e}, lse {el:.4e} / {yl:.4e}")
        assert eo <= 1.25 * yo and el <= 1.25 * yl


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_append_and_attention_in_one_graph(sa, pv):
    """{append; the one-launch attention} captured once; the lengths are then changed and the table is rewritten in place --
    two sequences trade their pages, the entry that left the window names the spare page -- and every replay equals the eager
    call on the new values"""
    cache, table, lens, spare = _setup.__wrapped__(128, pv, torch.float16, "per_thread", 64)
    _, qf = _rand_q(1, 4, 128, torch.float16)
    sinks = _sinks(4)

    def step():
        cache.append(table, lens, lens, 1)
        return sa.sageattn_decode_paged_window(qf, cache, table, lens, 100, num_splits=1, q_fold=4, sinks=sinks, return_lse=True)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og, lg = step()
    lens.copy_(torch.tensor([3, 0, 60, 64, 1, 200, 65, 100], dtype=torch.int32).cuda())
    table[[5, 7]] = table[[7, 5]]
    table[5, :(200 - 1 - 100 + 1) // 64] = spare
    oe, le = step()
    for _ in range(3):
        og.fill_(1.0); lg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same((og, lg), (oe, le))


def test_compile_fullgraph(sa):
    cache, table, lens, _ = _setup(64, "fp8", torch.float16, "per_thread", 64)
    _, qf = _rand_q(3, 4, 64, torch.float16)
    sinks = _sinks(4)
    torch.compiler.reset()
    got = torch.compile(lambda qq, tab, ln: sa.sageattn_decode_paged_window_compilable(qq, cache, tab, ln, 100, 1, 4, sinks,
                                                                                       return_lse=True),
                        backend="aot_eager", fullgraph=True)(qf, table, lens)
    torch.cuda.synchronize()
    assert _same(got, sa.sageattn_decode_paged_window(qf, cache, table, lens, 100, num_splits=1, q_fold=4, sinks=sinks, return_lse=True))
