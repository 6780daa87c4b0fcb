"""Sliding-window attention and sink logits on the paged cache on the GPU (``sageattn_splitkv_paged_window`` and its ragged form,
include/sageattn_hip_window.h): the window is exactly the window on constructed operands, the bit anchors against the parent
operators, random data against a plain float64 softmax, pages that have left the window, one HIP graph and torch.compile."""
import functools
import itertools

import pytest
import torch

import paged_util as PU

pytestmark = pytest.mark.gpu

HQ, HK = 4, 2
LENS = (300, 131, 64, 5, 0, 320)
LONG = (1000, 900)               # with window 700 and T 70: a left prologue, then RING + 2 or more tiles of the fast loop
RAGGED_T = (70, 1, 5, 5, 5, 1)   # a 70-token chunk, decode rows, a chunk as long as its cache, a sequence without keys
WINDOWS = (1, 7, 64, 100, 129, 4096)
SINKS = (0.5, -1.0, 2.0, 0.0)    # one value per query head
COMBOS = ((64, "fp16"), (64, "fp8"), (128, "fp16"), (128, "fp8"))


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    return sageattention_amd


@functools.lru_cache(maxsize=None)
def _setup(D, pv, page_size=64, onehot=False, gran="per_thread", LENS=LENS, dtype=torch.float16):
    """-> (cache, table, lens, spare): random pools (onehot: V[j, c] = 1 iff j mod D == c, exact in fp16 and, with v_headroom 2,
    in e4m3) behind a permuted table; ``spare`` is a valid page no row names, its state overwritten with NaN and garbage"""
    import sageattention_amd as sa
    max_pages = -(-max(320, *LENS) // page_size)
    k, v, P = PU.make_pools(24 if max(LENS) <= 320 else 40, HK, page_size, D, "HND", dtype, "cuda", seed=D + page_size)
    table = PU.make_table(LENS, max_pages, page_size, P, P, seed=5)
    if onehot:
        for b, n in enumerate(LENS):
            for i in range(PU.pages_needed(n, page_size)):
                j = i * page_size + torch.arange(page_size, device="cuda")
                v[int(table[b, i])] = torch.nn.functional.one_hot(j % D, D).to(dtype)
    else:
        PU.poison_tails(k, v, table, LENS, "HND")
    lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    cache = sa.SagePagedKVCache.prepare(k, v, table.cuda(), lens, pv=pv, qk_quant_gran=gran, v_headroom=2.0)
    used = {int(table[b, i]) for b, n in enumerate(LENS) for i in range(PU.pages_needed(n, page_size))}
    spare = min(set(range(P)) - used)
    cache.k8[spare] = 127
    cache.k_scale[spare] = float("nan")
    k[spare] = float("nan")
    v[spare] = float("nan")
    if pv == "fp8":
        cache.v8.view(torch.uint8)[spare] = 0x7f
    return cache, table.cuda(), lens, spare


def _bits(x):
    return x.view(torch.int16) if x.element_size() == 2 else x.view(torch.int32)


def _fold(q, g):      # [B, T, HQ, D] -> [B, HQ / g, T * g, D]
    B, T, _, D = q.shape
    return q.reshape(B, T, HQ // g, g, D).permute(0, 2, 1, 3, 4).reshape(B, HQ // g, T * g, D)


def _unfold(x, g):    # [B, HQ / g, T * g, ...] -> [B, T, HQ, ...]
    B, T = x.size(0), x.size(2) // g
    return x.reshape(B, HQ // g, T, g, *x.shape[3:]).transpose(1, 2).reshape(B, T, HQ, *x.shape[3:])


def _allowed(T, n, window):
    """bool [T, n]: the keys token t of T, the last positions of n keys, attends"""
    j, lim = torch.arange(n).view(1, n), torch.arange(T).view(T, 1) + (n - T)
    return (j <= lim) & (j >= lim - window + 1)


def _check_constructed(o, lse, Ts, window, D, sinks, LENS):
    """o [tokens, HQ, D], lse [tokens, HQ] against count and n_c of the rule, all sequences.  The bound on o is the issue's for
    fp16 (2^-10, twice the half-ulp of 11 significand bits) and the same multiple for bf16's 8 bits, 2^-7"""
    rel = 2.0 ** -10 if o.dtype == torch.float16 else 2.0 ** -7
    al = [_allowed(T, n, window).double() for T, n in zip(Ts, LENS)]
    count = torch.cat([a.sum(1) for a in al]).view(-1, 1)
    n_c = torch.cat([a @ torch.nn.functional.one_hot(torch.arange(n) % D, D).double() for a, n in zip(al, LENS)])
    den = count + (torch.tensor(sinks, dtype=torch.float64).exp().view(1, HQ) if sinks else 0.0) * (count > 0)
    o, lse = o.double().cpu(), lse.double().cpu()
    has = (count > 0).expand(-1, HQ)
    assert torch.equal(torch.isfinite(lse), has) and bool(torch.isneginf(lse[~has]).all()) and bool((o[~has] == 0).all())
    want_l = den.expand(-1, HQ)[has].log()
    assert float((lse[has] - want_l).abs().max()) <= 1e-5
    want_o = (n_c.unsqueeze(1) / den.clamp(min=1).unsqueeze(-1)).expand(-1, HQ, -1)
    assert bool(((o - want_o).abs() <= rel * want_o + 1e-6)[has].all())


# every (D, pv) meets every (S, g) over the windows; per-warp K scales at every other window
GRID = [(w, S, g) + COMBOS[(i + i // 4) % 4] + (64, ("per_thread", "per_warp")[i // 4 % 2], LENS, torch.float16)
        for i, (w, S, g) in enumerate(itertools.product(WINDOWS, (1, 3), (1, 2)))]
GRID.append((100, 3, 2, 128, "fp8", 128, "per_thread", LENS, torch.float16))
GRID += [(700, 1, g, D, pv, 64, ("per_thread", "per_warp")[g - 1], LONG, torch.float16) for g in (1, 2) for D, pv in COMBOS]
GRID += [(700, 1, 1, 64, "fp16", 64, "per_thread", LONG, torch.bfloat16), (100, 3, 2, 128, "fp16", 64, "per_warp", LENS, torch.bfloat16)]


@pytest.mark.parametrize("window,S,g,D,pv,page_size,gran,lens_c,dtype", GRID, ids=lambda x: str(x))
def test_the_window_is_exactly_the_window(sa, window, S, g, D, pv, page_size, gran, lens_c, dtype):
    cache, table, lens, _ = _setup(D, pv, page_size, True, gran, lens_c, dtype)
    B, Ts = len(lens_c), RAGGED_T[:len(lens_c)]
    for T, sinks in itertools.product((1, 5, 70), (None, SINKS)):
        st = None if sinks is None else torch.tensor(sinks, device="cuda")
        q = torch.zeros(B, HQ // g, T * g, D, dtype=dtype, device="cuda")
        o, lse = sa.sageattn_splitkv_paged_window(q, cache, table, lens, window, num_splits=S, q_fold=g, sinks=st, return_lse=True)
        _check_constructed(_unfold(o, g).reshape(B * T, HQ, D), _unfold(lse, g).reshape(B * T, HQ), (T,) * B, window, D, sinks, lens_c)
    cu = torch.tensor([0] + list(itertools.accumulate(Ts)), dtype=torch.int32, device="cuda")
    q = torch.zeros(sum(Ts), HQ, D, dtype=dtype, device="cuda")
    for sinks in (None, SINKS):
        st = None if sinks is None else torch.tensor(sinks, device="cuda")
        o, lse = sa.sageattn_splitkv_paged_ragged_window(q, cache, table, lens, cu, window, num_splits=S, q_fold=g, sinks=st,
                                                         return_lse=True)
        _check_constructed(o, lse, Ts, window, D, sinks, lens_c)


def _rand_q(B, T, D, g):
    q = torch.randn(B, T, HQ, D, generator=torch.Generator().manual_seed(11)).to(torch.float16).cuda()
    return q, _fold(q, g)


@pytest.mark.parametrize("T,S,g", [(1, 1, 1), (5, 1, 2), (70, 1, 1), (70, 1, 2), (5, 3, 1), (5, 3, 2)])
@pytest.mark.parametrize("D,pv", COMBOS)
def test_anchor_a_wide_window_has_the_parents_bits(sa, D, pv, T, S, g):     # (a) S = 1, (b) T = 5 and S = 3
    cache, table, lens, _ = _setup(D, pv)
    _, qf = _rand_q(len(LENS), T, D, g)
    o, lse = sa.sageattn_splitkv_paged_window(qf, cache, table, lens, 4096, num_splits=S, q_fold=g, return_lse=True)
    po, pl = sa.sageattn_splitkv_paged(qf, cache, table, lens, num_splits=S, causal=True, q_fold=g, return_lse=True)
    assert torch.equal(_bits(o), _bits(po)) and torch.equal(_bits(lse), _bits(pl))


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("D,pv", COMBOS)
def test_anchor_c_decode_has_the_bits_of_the_shifted_table(sa, D, pv, S):
    cache, table, lens, _ = _setup(D, pv)
    one = cache.narrow(5, 1)                                                  # the sequence of 320 keys
    _, qf = _rand_q(1, 1, D, 2)
    o, lse = sa.sageattn_splitkv_paged_window(qf, one, table[5:6], lens[5:6], 128, num_splits=S, q_fold=2, return_lse=True)
    shifted = table[5:6, (320 - 128) // 64:].contiguous()
    po, pl = sa.sageattn_splitkv_paged(qf, one, shifted, torch.full_like(lens[5:6], 128), num_splits=S, causal=True, q_fold=2,
                                       return_lse=True)
    assert torch.equal(_bits(o), _bits(po)) and torch.equal(_bits(lse), _bits(pl))


@pytest.mark.parametrize("D,pv", COMBOS)
def test_anchor_d_ragged_rows_have_the_bits_of_the_per_sequence_call(sa, D, pv):
    cache, table, lens, _ = _setup(D, pv)
    cu = [0] + list(itertools.accumulate(RAGGED_T))
    q = torch.randn(cu[-1], HQ, D, generator=torch.Generator().manual_seed(3)).to(torch.float16).cuda()
    st = torch.tensor(SINKS, device="cuda")
    o, lse = sa.sageattn_splitkv_paged_ragged_window(q, cache, table, lens, torch.tensor(cu, dtype=torch.int32, device="cuda"),
                                                     100, num_splits=3, q_fold=2, sinks=st, return_lse=True)
    for b, T in enumerate(RAGGED_T):
        po, pl = sa.sageattn_splitkv_paged_window(_fold(q[cu[b]:cu[b + 1]].unsqueeze(0), 2), cache.narrow(b, 1), table[b:b + 1],
                                                  lens[b:b + 1], 100, num_splits=3, q_fold=2, sinks=st, return_lse=True)
        assert torch.equal(_bits(o[cu[b]:cu[b + 1]]), _bits(_unfold(po, 2)[0]))
        assert torch.equal(_bits(lse[cu[b]:cu[b + 1]]), _bits(_unfold(pl, 2)[0]))


def _float64_rule(cache, table, q, window):
    """softmax in float64 over the fp16 K / V gathered from the pages, keys t + off - window + 1 <= j <= t + off; no operator of
    the library.  q [B, T, HQ, D] -> o [B, T, HQ, D], lse [B, T, HQ] (a row without keys: o = 0, lse = -inf)"""
    kg, vg = PU.gather(cache.k, table, "HND").double(), PU.gather(cache.v, table, "HND").double()    # [B, Hk, N, D]
    B, T, _, D = q.shape
    o = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    lse = torch.full(q.shape[:3], float("-inf"), dtype=torch.float64, device=q.device)
    for b, n in enumerate(LENS):
        if n:
            kk, vv = (x[b, :, :n].repeat_interleave(HQ // HK, dim=0) for x in (kg, vg))            # [HQ, n, D]
            s = q[b].double().transpose(0, 1) @ kk.transpose(1, 2) * D ** -0.5                      # [HQ, T, n]
            s = s.masked_fill(~_allowed(T, n, window).to(q.device), float("-inf"))
            l = torch.logsumexp(s, dim=-1)
            p = torch.exp(s - torch.where(torch.isneginf(l), torch.zeros_like(l), l).unsqueeze(-1))
            o[b], lse[b] = (p @ vv).transpose(0, 1), l.transpose(0, 1)
    return o, lse


def _errors(o, lse, o64, l64):
    fin = torch.isfinite(l64)
    assert torch.equal(torch.isfinite(lse), fin) and bool(torch.isneginf(lse[~fin]).all())
    return float((o.double() - o64).abs().max()), float((lse.double()[fin] - l64[fin]).abs().max())


@pytest.mark.parametrize("window", [100, 129])
@pytest.mark.parametrize("D,pv", COMBOS)
def test_random_data_against_float64(sa, D, pv, window):
    """The yardstick is the existing causal operator's own error against its float64 rule on the same cache and queries, measured
    in this run; the window call may reach twice that (its rows average over fewer keys).  Measured: profiles/window.md."""
    cache, table, lens, _ = _setup(D, pv)
    q, qf = _rand_q(len(LENS), 70, D, 2)
    po, pl = sa.sageattn_splitkv_paged(qf, cache, table, lens, num_splits=3, causal=True, q_fold=2, return_lse=True)
    yo, yl = _errors(_unfold(po, 2), _unfold(pl, 2), *_float64_rule(cache, table, q, 10 ** 6))
    o, lse = sa.sageattn_splitkv_paged_window(qf, cache, table, lens, window, num_splits=3, q_fold=2, return_lse=True)
    eo, el = _errors(_unfold(o, 2), _unfold(lse, 2), *_float64_rule(cache, table, q, window))
    print(f"window={window} D={D} pv={pv}: max|o - o64| = {eo:.4e} (parent {yo:.4e}), max|lse - lse64| = {el:.4e} (parent {yl:.4e})")
    assert eo <= 2 * yo and el <= 2 * yl


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("D,pv", COMBOS)
def test_pages_that_left_the_window_are_not_touched(sa, D, pv, T):
    cache, table, lens, spare = _setup(D, pv)
    _, qf = _rand_q(len(LENS), T, D, 2)
    freed = table.clone()
    for b, n in enumerate(LENS):
        freed[b, :max(n - T - 100 + 1, 0) // 64] = spare
    assert int((freed != table).sum()) >= 6
    st = torch.tensor(SINKS, device="cuda")
    kw = dict(num_splits=3, q_fold=2, sinks=st, return_lse=True)
    o, lse = sa.sageattn_splitkv_paged_window(qf, cache, table, lens, 100, **kw)
    fo, fl = sa.sageattn_splitkv_paged_window(qf, cache, freed, lens, 100, **kw)
    assert torch.equal(_bits(o), _bits(fo)) and torch.equal(_bits(lse), _bits(fl)) and bool(torch.isfinite(fo).all())


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_append_and_attention_in_one_graph(sa, pv):
    """{append; window attention} captured once; kv_lens and the table are then rewritten in place and every replay equals the
    eager call on the new values"""
    cache, table, lens, spare = _setup.__wrapped__(128, pv)                    # a cache of its own: the append writes state
    table, lens = table.clone(), lens.clone()
    _, qf = _rand_q(len(LENS), 5, 128, 2)
    st = torch.tensor(SINKS, device="cuda")

    def step():
        cache.append(table, lens, lens, 1)
        return sa.sageattn_splitkv_paged_window(qf, cache, table, lens, 100, num_splits=3, q_fold=2, sinks=st, return_lse=True)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og, lg = step()
    lens.copy_(torch.tensor([260, 100, 64, 3, 0, 300], dtype=torch.int32).cuda())
    table[0, :2] = spare                                                       # (260 - 5 - 100 + 1) // 64 entries have left
    oe, le = step()
    for _ in range(3):
        og.fill_(1.0); lg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(og), _bits(oe)) and torch.equal(_bits(lg), _bits(le))


def test_compile_fullgraph(sa):
    cache, table, lens, _ = _setup(64, "fp8")
    _, qf = _rand_q(len(LENS), 5, 64, 2)
    st = torch.tensor(SINKS, device="cuda")

    def step(qq, tab, ln, sk):
        return torch.ops.sageattention_amd_window.attn_splitkv_paged_window_lse(
            qq, cache.k8, cache.k_scale, cache.km, cache.v8, cache.v_scale, tab, ln, 3, 2, 100, sk, "HND", 0.125, "per_thread")

    torch.compiler.reset()
    oc, lc = torch.compile(step, backend="aot_eager", fullgraph=True)(qf, table, lens, st)
    oe, le = sa.sageattn_splitkv_paged_window(qf, cache, table, lens, 100, num_splits=3, q_fold=2, sinks=st, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(oc), _bits(oe)) and torch.equal(_bits(lc), _bits(le))
