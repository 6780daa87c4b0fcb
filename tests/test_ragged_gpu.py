"""Ragged-query attention on the paged cache on the GPU (``sageattn_splitkv_paged_ragged``, include/sageattn_hip_ragged.h): every
sequence's rows against ``sageattn_splitkv_paged(causal=True)`` on that sequence alone, bit for bit; the rule against a plain
float64 softmax; {plan; attention} in one HIP graph; the ops under torch.compile.  One batch (SEQS) holds every edge."""
import functools
import itertools

import pytest
import torch

import paged_util as PU

pytestmark = pytest.mark.gpu

HQ, HK = 4, 2
SEQS = ((1, 200), (0, 70), (67, 67), (3, 2), (5, 0), (128, 320))  # (T_b, len_b): decode; no tokens; prefill; chunk > cache; no keys; full
FAR = 2 ** 30  # a table entry no kernel may follow


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    return sageattention_amd


def _cu(seqs):
    return torch.tensor([0] + list(itertools.accumulate(t for t, _ in seqs)), dtype=torch.int32)


def _call_table(table, seqs, page_size):
    """the table of the attention calls: FAR behind each row's valid entries and in the whole row of a sequence without tokens"""
    t = table.clone()
    for b, (T, n) in enumerate(seqs):
        t[b, 0 if T == 0 else PU.pages_needed(n, page_size):] = FAR
    return t


@functools.lru_cache(maxsize=None)
def _setup(D, pv, gran, page_size):
    """-> (cache, the table it was prepared with, the table of the calls, lens, cu, q, q's buffer): pools with NaN rows behind
    len_b, a permuted table, q a strided view inside a NaN-filled buffer"""
    import sageattention_amd as sa
    max_pages = 320 // page_size + (320 % page_size != 0)
    lens = [n for _, n in SEQS]
    k, v, P = PU.make_pools(16, HK, page_size, D, "HND", torch.float16, "cuda", seed=D + page_size)
    table = PU.make_table(lens, max_pages, page_size, P, P, seed=3, reverse_row=5)
    PU.poison_tails(k, v, table, lens, "HND")
    lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    cache = sa.SagePagedKVCache.prepare(k, v, table.cuda(), lens_t, pv=pv, qk_quant_gran=gran)
    T = sum(t for t, _ in SEQS)
    buf = torch.full((T + 2, HQ + 2, 2 * D), float("nan"), dtype=torch.float16, device="cuda")
    q = buf[1:T + 1, 1:HQ + 1, D:]
    q.copy_(torch.randn(T, HQ, D, generator=torch.Generator().manual_seed(7)).to(torch.float16))
    return cache, table, _call_table(table, SEQS, page_size).cuda(), lens_t, _cu(SEQS).cuda(), q, buf


def _per_sequence(sa, cache, table, lens_t, cu, q, g, S):
    """the existing operator on each sequence alone, q folded by hand and the result un-folded -> o [T, Hq, D], lse [T, Hq]
    (rows of no sequence keep NaN)"""
    o = torch.full(q.shape, float("nan"), dtype=q.dtype, device=q.device)
    lse = torch.full(q.shape[:2], float("nan"), dtype=torch.float32, device=q.device)
    D = q.size(-1)
    for b in range(cu.numel() - 1):
        lo, hi = int(cu[b]), int(cu[b + 1])
        T = hi - lo
        if T == 0:
            continue
        qb = q[lo:hi].reshape(T, HQ // g, g, D).permute(1, 0, 2, 3).reshape(1, HQ // g, T * g, D)
        ob, lb = sa.sageattn_splitkv_paged(qb, cache.narrow(b, 1), table[b:b + 1], lens_t[b:b + 1], num_splits=S, causal=True,
                                           q_fold=g, return_lse=True)
        o[lo:hi] = ob.reshape(HQ // g, T, g, D).permute(1, 0, 2, 3).reshape(T, HQ, D)
        lse[lo:hi] = lb.reshape(HQ // g, T, g).permute(1, 0, 2).reshape(T, HQ)
    return o, lse


def _bits(x):
    return x.view(torch.int16) if x.element_size() == 2 else x.view(torch.int32)


_POINTS = list(itertools.product((64, 128), ("fp16", "fp8"), (1, 2), (1, 3)))
CASES = [(D, pv, g, S, ("per_thread", "per_warp")[i % 2], 64) for i, (D, pv, g, S) in enumerate(_POINTS)]
CASES.append((128, "fp8", 2, 3, "per_thread", 128))


@pytest.mark.parametrize("D,pv,g,S,gran,page_size", CASES, ids=lambda x: str(x))
def test_rows_have_the_bits_of_the_per_sequence_operator(sa, D, pv, g, S, gran, page_size):
    cache, _, table, lens_t, cu, q, buf = _setup(D, pv, gran, page_size)
    before = buf.clone()
    plan = sa.ragged_q_plan(cu, q.size(0), g)
    o, lse = sa.sageattn_splitkv_paged_ragged(q, cache, table, lens_t, cu, plan=plan, num_splits=S, q_fold=g, return_lse=True)
    o2 = sa.sageattn_splitkv_paged_ragged(q, cache, table, lens_t, cu, num_splits=S, q_fold=g)   # the plan made inside, no lse
    ro, rl = _per_sequence(sa, cache, table, lens_t, cu, q, g, S)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.is_contiguous() and o.dtype == q.dtype and lse.shape == q.shape[:2]
    assert torch.equal(_bits(o), _bits(ro)) and torch.equal(_bits(lse), _bits(rl)) and torch.equal(_bits(o2), _bits(o))
    assert torch.equal(_bits(buf), _bits(before))                      # q is read in place: its buffer is what it was
    # the list: one pair per q-block that exists, in sequence order, then b = -1
    want = [(b, i) for b, (T, _) in enumerate(SEQS) for i in range((T * g + 127) // 128)]
    items = plan.items.cpu().tolist()
    assert len(items) == q.size(0) * g // 128 + len(SEQS) and [tuple(x) for x in items[:len(want)]] == want
    assert all(b == -1 for b, _ in items[len(want):])
    # the defined rows: a sequence without keys, and the first token of the chunk that is longer than its cache
    c = cu.tolist()
    assert bool((o[c[4]:c[5]] == 0).all()) and bool(torch.isneginf(lse[c[4]:c[5]]).all())
    assert bool((o[c[3]] == 0).all()) and bool(torch.isneginf(lse[c[3]]).all()) and bool(torch.isfinite(lse[c[3] + 1]).all())


def _float64_rule(cache_k, cache_v, table, q, D):
    """per-sequence softmax in float64 over the fp16 K / V gathered from the pages, mask j <= t + len_b - T_b; no operator of the
    library -> o [T, Hq, D], lse [T, Hq] (natural log; a row without keys: o = 0, lse = -inf)"""
    kg, vg = PU.gather(cache_k, table, "HND").double(), PU.gather(cache_v, table, "HND").double()    # [B, Hk, N, D]
    o = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    lse = torch.full(q.shape[:2], float("-inf"), dtype=torch.float64, device=q.device)
    lo = 0
    for b, (T, n) in enumerate(SEQS):
        if T and n:
            qq = q[lo:lo + T].double().permute(1, 0, 2)                                             # [Hq, T, D]
            kk, vv = (x[b, :, :n].repeat_interleave(HQ // HK, dim=0) for x in (kg, vg))            # [Hq, n, D]
            s = qq @ kk.transpose(1, 2) * D ** -0.5
            allowed = torch.arange(n, device=q.device).view(1, 1, n) <= torch.arange(T, device=q.device).view(1, T, 1) + (n - T)
            s = s.masked_fill(~allowed, float("-inf"))
            l = torch.logsumexp(s, dim=-1)                                                          # [Hq, T]
            p = torch.exp(s - torch.where(torch.isneginf(l), torch.zeros_like(l), l).unsqueeze(-1))
            o[lo:lo + T] = (p @ vv).permute(1, 0, 2)
            lse[lo:lo + T] = l.permute(1, 0)
        lo += T
    return o, lse


# max |o - o64| and max |lse - lse64| of the parent's sageattn_splitkv_paged(causal=True), called per sequence on this batch
# (g = 2, S = 3, per_thread), against _float64_rule: measured on an MI355X, profiles/ragged_q.md.  The tolerance is 1.5 times
# them: the margin is for a later change of seed or shape -- the bits themselves are equal by the test above.
PARENT_ERR = {(64, "fp16"): (4.289347e-02, 3.485046e-02), (64, "fp8"): (9.960938e-02, 3.486667e-02),
              (128, "fp16"): (4.852744e-02, 4.003028e-02), (128, "fp8"): (1.096368e-01, 4.003463e-02)}


def _errors(o, lse, o64, l64):
    fin = torch.isfinite(l64)
    assert torch.equal(torch.isfinite(lse), fin) and bool(torch.isneginf(lse[~fin]).all())
    return float((o.double() - o64).abs().max()), float((lse.double()[fin] - l64[fin]).abs().max())


@pytest.mark.parametrize("D,pv", list(PARENT_ERR), ids=lambda x: str(x))
def test_the_rule_against_float64(sa, D, pv):
    cache, prep_table, table, lens_t, cu, q, _ = _setup(D, pv, "per_thread", 64)
    o64, l64 = _float64_rule(cache.k, cache.v, prep_table, q, D)
    o, lse = sa.sageattn_splitkv_paged_ragged(q, cache, table, lens_t, cu, num_splits=3, q_fold=2, return_lse=True)
    eo, el = _errors(o, lse, o64, l64)
    print(f"ragged D={D} pv={pv}: max|o - o64| = {eo:.4e}, max|lse - lse64| = {el:.4e}; parent {PARENT_ERR[(D, pv)]}")
    po, pl = PARENT_ERR[(D, pv)]
    assert eo <= 1.5 * po and el <= 1.5 * pl


def _other_division(page_size=64):
    """another division of the same 204 tokens over the 6 sequences (lengths within what the prepared pages hold)"""
    seqs = ((40, 200), (3, 70), (0, 67), (1, 2), (32, 0), (128, 200))
    assert sum(t for t, _ in seqs) == sum(t for t, _ in SEQS) and all(n <= m for (_, n), (_, m) in zip(seqs, SEQS))
    return seqs


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_plan_and_attention_in_one_graph(sa, pv):
    """{ragged_q_plan; attention} captured once; cu_seqlens_q, kv_lens and the table are then overwritten in place with another
    division of the same total_tokens, and every replay equals the eager call on the new values"""
    cache, prep_table, table, lens_t, cu, q, _ = _setup(128, pv, "per_thread", 64)
    table, lens_t, cu = table.clone(), lens_t.clone(), cu.clone()

    def step():
        plan = sa.ragged_q_plan(cu, q.size(0), 2)
        return sa.sageattn_splitkv_paged_ragged(q, cache, table, lens_t, cu, plan=plan, num_splits=3, q_fold=2, return_lse=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og, lg = step()
    seqs = _other_division()
    cu.copy_(_cu(seqs).cuda())
    lens_t.copy_(torch.tensor([n for _, n in seqs], dtype=torch.int32).cuda())
    table.copy_(_call_table(prep_table, seqs, 64).cuda())
    oe, le = step()
    for _ in range(3):
        og.fill_(1.0); lg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(og), _bits(oe)) and torch.equal(_bits(lg), _bits(le))
    ro, rl = _per_sequence(sa, cache, table, lens_t, cu, q, 2, 3)
    assert torch.equal(_bits(oe), _bits(ro)) and torch.equal(_bits(le), _bits(rl))


def test_compile_fullgraph(sa):
    cache, _, table, lens_t, cu, q, _ = _setup(64, "fp8", "per_warp", 64)
    ops = torch.ops.sageattention_amd_ragged

    def step(qq, tab, lens, cuq):
        items = ops.ragged_q_plan(cuq, qq.size(0), 2)
        return ops.attn_splitkv_paged_ragged_lse(qq, cache.k8, cache.k_scale, cache.km, cache.v8, cache.v_scale, tab, lens, cuq,
                                                 items, 3, 2, "HND", 0.125, "per_warp")

    torch.compiler.reset()
    oc, lc = torch.compile(step, backend="aot_eager", fullgraph=True)(q, table, lens_t, cu)
    oe, le = sa.sageattn_splitkv_paged_ragged(q, cache, table, lens_t, cu, num_splits=3, q_fold=2, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(oc), _bits(oe)) and torch.equal(_bits(lc), _bits(le))
