"""The paged MXFP4 V cache on the GPU (``SagePagedKVCacheV4``, ``sageattn_splitkv_paged_v4``; the rule:
include/sageattn_hip_paged_fp4.h).  Paging is an addressing change, so the checks are ``torch.equal`` against code that exists
without it -- ``SageKVCacheV4`` / ``sageattn_splitkv_v4`` on the padded tensors gathered from the pages (tests/paged_util.py),
taken through the same appends -- and, once per (head_dim, page size), the float64 bound of test_fp4_gpu.py.

Every pool row no sequence holds is NaN (unnamed pages, the poison page the unused table entries name, rows at or beyond
len_b), and the image pools of unnamed pages are 0xFF: a wrong read shows as wrong bits, never as a fault."""
import itertools

import pytest
import torch

import kvcache_util as KU
import paged_util as PU
import sageattention_amd as sa
from conftest import softmax_weights
from oracle import sage_oracle as O
from splitkv_causal_util import allowed_keys
from test_fp4_gpu import STEPS, decode

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _hand_memory_back():
    """NaN rows and poison bytes on purpose: the cached blocks go back to the driver, as in test_fp4_gpu.py"""
    yield
    _CASES.clear()
    torch.cuda.empty_cache()


def _lens(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


class Pools:
    """fp16 pools of all-NaN rows, a permuted table for ``lens_max`` (unused entries: the poison page), and the sequences'
    logical rows ``kl`` / ``vl`` [B,Hk,N,D]; ``write`` is the caller putting rows [start_b, len_b) into the pages, after which
    ``kg`` / ``vg`` hold the tensors gathered from the pages (the reference cache binds them)"""

    def __init__(self, D, ps, layout, lens_max, N, Hk, seed):
        self.ps, self.layout, self.lens_max = ps, layout, lens_max
        P = sum(PU.pages_needed(n, ps) for n in lens_max) + 3     # more pages than the table names
        self.k_pool, self.v_pool, poison = PU.make_pools(P, Hk, ps, D, layout, torch.float16, "cuda", seed)
        self.k_pool.fill_(NAN)
        self.v_pool.fill_(NAN)
        self.table_cpu = PU.make_table(lens_max, N // ps, ps, P, poison, seed=seed)
        self.table = self.table_cpu.cuda()
        named = {int(p) for b, n in enumerate(lens_max) for p in self.table_cpu[b, :PU.pages_needed(n, ps)]}
        self.unnamed = sorted(set(range(P + 1)) - named)
        self.kl, self.vl = (torch.full((len(lens_max), Hk, N, D), NAN, dtype=torch.float16) for _ in range(2))
        self.kg, self.vg = (PU.gather(p, self.table_cpu, layout) for p in (self.k_pool, self.v_pool))

    def write(self, start, lens, g):
        B, Hk, N, D = self.kl.shape
        for x, pool, out, amp in ((self.kl, self.k_pool, self.kg, 1.5), (self.vl, self.v_pool, self.vg, 3.0)):
            for b, (s, n) in enumerate(zip(start, lens)):
                if n > s:
                    x[b, :, s:n] = (torch.randn(Hk, n - s, D, generator=g) * amp).half()
                x[b, :, n:] = NAN                                  # (a rollback: the rows behind the length are poison again)
                need = PU.pages_needed(self.lens_max[b], self.ps)
                pages = x[b].view(Hk, N // self.ps, self.ps, D).transpose(0, 1)[:need].cuda()
                PU.hnd_pool(pool, self.layout)[self.table_cpu[b, :need].long().cuda()] = pages
            out.copy_(PU.gather(pool, self.table_cpu, self.layout))


def assert_valid_tiles_equal(cache, ref, table, lens):
    for what, got, want in PU.valid_tile_views(cache._kc, ref._kc, table, lens):     # INT8 rows < len_b and the K scales
        assert torch.equal(got, want), what
    for b, n in enumerate(lens):
        for t in range((n + 63) // 64):
            page, ti = PU.tile_home(table[b].tolist(), t, cache.page_size)
            assert torch.equal(cache.v4[page, :, :, 32 * ti:32 * ti + 32], ref.v4[b, :, :, 32 * t:32 * t + 32]), ("v4", b, t)
            assert torch.equal(cache.v4_scale[page, :, ti], ref.v4_scale[b, :, t]), ("v4_scale", b, t)


def state_and_touched(cache, table, start, lens):
    """the four state pools as CPU integer tensors (K in its HND view), and masks of what an append of (start, lens) may write"""
    state = (PU.hnd_pool(cache.k8, cache.tensor_layout).cpu(), cache.k_scale.view(torch.int32).cpu(), cache.v4.cpu(),
             cache.v4_scale.cpu())
    mk, ms, _ = PU.touched_masks(cache._kc, table, [(start, lens)])
    m4, m4s = torch.zeros(state[2].shape, dtype=torch.bool), torch.zeros(state[3].shape, dtype=torch.bool)
    for b, (s, n) in enumerate(zip(start, lens)):
        for t in KU.touched_tiles(s, n, table.shape[1] * cache.page_size):
            page, ti = PU.tile_home(table[b].tolist(), t, cache.page_size)
            m4[page, :, :, 32 * ti:32 * ti + 32] = True
            m4s[page, :, ti] = True
    return state, (mk, ms, m4, m4s)


# ---- 1. append equals the contiguous cache ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("HND", "NHD"))
@pytest.mark.parametrize("ps", (64, 256))
@pytest.mark.parametrize("D,gran", [(64, "per_thread"), (128, "per_thread"), (128, "per_warp")])
def test_append_equals_contiguous_cache(D, gran, ps, layout):
    """after ``prepare`` and after every step of test_fp4_gpu.py's STEPS every valid tile is the reference's, bit for bit, and
    every byte outside the touched tiles -- all unnamed pages included -- is what it was before the step"""
    w = Pools(D, ps, layout, (256, 256, 0), 256, 2, seed=D + ps)
    g = torch.Generator().manual_seed(7)
    w.write((0, 0, 0), STEPS[0][0], g)
    lens0 = _lens(STEPS[0][0])
    cache = sa.SagePagedKVCacheV4.prepare(w.k_pool, w.v_pool, w.table, lens0, gran, layout)
    ref = sa.SageKVCacheV4.prepare(w.kg, w.vg, lens0, gran, layout)
    cache.v4[w.unnamed] = 0xFF
    cache.v4_scale[w.unnamed] = 0xFF
    assert_valid_tiles_equal(cache, ref, w.table_cpu, STEPS[0][0])
    for start, lens in STEPS:
        w.write(start, lens, g)
        before, masks = state_and_touched(cache, w.table_cpu, start, lens)
        cache.append(w.table, _lens(start), _lens(lens), 70)
        ref.append(_lens(start), _lens(lens), 70)
        assert_valid_tiles_equal(cache, ref, w.table_cpu, lens)
        after, _ = state_and_touched(cache, w.table_cpu, start, lens)
        for name, a, b4, m in zip(("k8", "k_scale", "v4", "v4_scale"), after, before, masks):
            assert torch.equal(a[~m], b4[~m]), (name, start, lens)
            assert m[w.unnamed].sum() == 0


# ---- 2. attention equals the contiguous operator, and float64 -----------------------------------------------------------------------
_CASES = {}
LENS = {256: (0, 1, 128, 200), 1280: (0, 1, 1024, 1100)}


def _case(D, gran, ps, N):
    """one paged cache, its contiguous reference and the decode of its image per (D, gran, page size, capacity)"""
    if (D, gran, ps, N) not in _CASES:
        lens = LENS[N]
        w = Pools(D, ps, "HND", lens, N, 1, seed=N + D + ps)
        w.write((0, 0, 0, 0), lens, torch.Generator().manual_seed(N + D))
        cache = sa.SagePagedKVCacheV4.prepare(w.k_pool, w.v_pool, w.table, _lens(lens), gran)
        ref = sa.SageKVCacheV4.prepare(w.kg, w.vg, _lens(lens), gran)
        cache.v4[w.unnamed] = 0xFF
        cache.v4_scale[w.unnamed] = 0xFF
        _CASES[D, gran, ps, N] = (w, cache, ref, decode(ref.v4, ref.v4_scale)[0])
    return _CASES[D, gran, ps, N]


ATTN = [c for c in itertools.product((64, 128), ("per_thread", "per_warp"), (64, 256), (1, 16, 130), (256, 1280), (1, 2, 3),
                                     (0, 1, 4)) if c[6] == 0 or c[3] % c[6] == 0]


@pytest.mark.parametrize("D,gran,ps,M,N,S,fold", ATTN)
def test_attention_equals_contiguous_operator(D, gran, ps, M, N, S, fold):
    """o and lse are those of ``sageattn_splitkv_v4`` on the gathered cache, bit for bit.  For one case per (D, page size) o is
    also held against float64 ``W @ V'`` on the decode of the cache's own image, on EVERY element, with the bound of
    test_fp4_gpu.py::test_attention_against_float64 as it stands: min(2^-4 W|V'|, 6 sqrt(2^-8/3 W^2 V'^2)) + 2 * 2^-10 *
    max(|ref|, .25) -- one e4m3 rounding of P, derived there."""
    w, cache, ref, vprime = _case(D, gran, ps, N)
    lens, ln = LENS[N], _lens(LENS[N])
    q = torch.randn(4, 2, M, D, generator=torch.Generator().manual_seed(M)).half()
    causal = fold > 0
    o, lse = sa.sageattn_splitkv_paged_v4(q.cuda(), cache, w.table, ln, S, causal, max(fold, 1), return_lse=True)
    ro, rlse = sa.sageattn_splitkv_v4(q.cuda(), ref, ln, S, causal, max(fold, 1), return_lse=True)
    assert torch.equal(o.view(torch.int16), ro.view(torch.int16)) and torch.equal(lse.view(torch.int32), rlse.view(torch.int32))
    assert bool((o[0] == 0).all()) and bool((lse[0] == float("-inf")).all())                 # the sequence without keys
    if (gran, M, N, S, fold) != ("per_thread", 130, 1280, 3, 1):
        return
    o, km = o.cpu().double(), cache.km.cpu()
    for b, n in enumerate(lens):
        if n == 0:
            continue
        keep = allowed_keys(n, M, fold, n)
        rows = keep.any(1)
        q8, qs, k8, ks = O.per_thread_int8(q[b:b + 1], w.kl[b:b + 1, :, :n], km[b:b + 1].unsqueeze(2))
        W = softmax_weights(q8, k8, O.expand_q_scale(qs, M, gran), O.expand_k_scale(ks, n, gran), D ** -0.5 * 1.44269504)
        W = W[0].double() * keep
        W = W / W.sum(-1, keepdim=True).clamp(min=1e-300)
        V = vprime[b, :, :n]
        want = W @ V
        bound = torch.minimum(2.0 ** -4 * (W @ V.abs()), 6 * torch.sqrt((2.0 ** -8 / 3) * ((W * W) @ (V * V)))) \
            + 2 * 2.0 ** -10 * want.abs().clamp(min=0.25)
        ratio = ((o[b] - want).abs() / bound)[:, rows].max().item()
        print(f"b={b} len={n}: max |o - ref| / bound = {ratio:.3f}")
        assert ratio <= 1.0, (b, ratio)


# ---- 3. graph and compile --------------------------------------------------------------------------------------------------------
def _step_world():
    w = Pools(128, 64, "HND", (256, 128), 256, 2, seed=3)
    w.write((0, 0), (256, 128), torch.Generator().manual_seed(3))                             # every row the steps will reach
    q = torch.randn(2, 4, 4, 128, generator=torch.Generator().manual_seed(4)).half().cuda()
    return w, q, _lens((190, 63))


def test_graph_replay_after_pages_moved():
    """{append; attention} in one HIP graph, replayed after the table was permuted in place, the pages moved accordingly and
    the lengths grew: every replay equals the eager step on the new state"""
    w, q, lens = _step_world()
    cache, eager = (sa.SagePagedKVCacheV4.prepare(w.k_pool, w.v_pool, w.table, lens) for _ in range(2))
    start = lens.clone()

    def step(c):
        c.append(w.table, start, lens, 1)
        return sa.sageattn_splitkv_paged_v4(q, c, w.table, lens, 2, True, 4, return_lse=True)

    step(cache)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(cache)
    pools = (w.k_pool, w.v_pool, cache.k8, cache.k_scale, cache.v4, cache.v4_scale, eager.k8, eager.k_scale, eager.v4, eager.v4_scale)
    for i in range(3):
        perm = torch.randperm(w.k_pool.size(0), generator=torch.Generator().manual_seed(i)).cuda()   # page p moves to perm[p]
        for t in pools:
            t[perm] = t.clone()
        w.table.copy_(perm[w.table.long()].int())
        start.copy_(lens)
        lens.add_(1)
        graph.replay()
        want = step(eager)
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
        assert torch.equal(cache.v4, eager.v4) and torch.equal(cache.v4_scale, eager.v4_scale)


def test_compile_fullgraph_equals_eager():
    w, q, lens = _step_world()
    cache, eager = (sa.SagePagedKVCacheV4.prepare(w.k_pool, w.v_pool, w.table, lens) for _ in range(2))
    ops = torch.ops.sageattention_amd_paged_fp4

    def step(q, k, v, km, k8, ks, v4, v4s, table, start, lens):
        ops.kv_cache_append_paged_v4(k, v, km, k8, ks, v4, v4s, table, start, lens, 1, "HND", "per_thread")
        return ops.attn_splitkv_paged_v4_lse(q, k8, ks, km, v4, v4s, table, lens, 2, "HND", 128 ** -0.5, "per_thread")

    args = lambda c: (q, w.k_pool, w.v_pool, c.km, c.k8, c.k_scale, c.v4, c.v4_scale, w.table, lens - 1, lens)  # noqa: E731
    o, lse = torch.compile(step, fullgraph=True)(*args(cache))
    o_e, lse_e = step(*args(eager))
    assert torch.equal(o, o_e) and torch.equal(lse, lse_e) and torch.equal(cache.v4, eager.v4)
