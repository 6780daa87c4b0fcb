"""The MXFP4 V image of the KV cache on the GPU (sageattention_amd/fp4.py; include/sageattn_hip_fp4.h holds the rule): the
quantizer against the rule restated in torch, the append against a from-scratch quantization, attention against float64
``W @ V'`` on the decode of the cache's own image, and the graph / compile forms against the eager calls."""
import itertools

import pytest
import torch

import sageattention_amd as sa
from conftest import softmax_weights
from oracle import sage_oracle as O
from splitkv_causal_util import allowed_keys

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _hand_memory_back():
    """This module fills device memory with NaN rows, poison bytes and random nibbles on purpose.  Its cached blocks go back to
    the driver afterwards, so that a later test's ``torch.empty`` does not get them: some compare never-written memory."""
    yield
    _CACHES.clear()
    torch.cuda.empty_cache()
GRID = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6], dtype=torch.float64)
_J = torch.arange(32)
TOKEN = ((_J & 3) + 8 * ((_J & 15) >> 2) + 4 * (_J >> 4)).view(1, 32) + 32 * torch.arange(2).view(2, 1)  # kv(hh, j)


# ---- the shared helper: the rule restated.  decode: image + scale bytes -> (V' float64 [B,H,64T,D], E [B,H,T,2,D]);
# quant_ref: v float64 [B,H,N,D] and lengths -> the same pair by the rule of the header ------------------------------------------
def decode(img, scale):
    img, scale = img.cpu(), scale.cpu()
    B, H, D, T = *img.shape[:3], scale.shape[2]
    by = img.view(B, H, D, T, 2, 16).long()
    nib = torch.stack((by & 15, by >> 4), -1).reshape(B, H, D, T, 2, 32)          # element j of lane half hh
    E = scale.view(B, H, T, 2, 32, D // 32).long().transpose(4, 5).reshape(B, H, T, 2, D)  # [hh][c % 32][c / 32] -> c
    val = GRID[nib & 7] * (1 - 2 * (nib >> 3)) * torch.exp2(E.permute(0, 1, 4, 2, 3).double() - 127).unsqueeze(-1)
    out = torch.zeros(B, H, D, T, 64, dtype=torch.float64)
    out[..., TOKEN.reshape(-1)] = val.reshape(B, H, D, T, 64)
    return out.reshape(B, H, D, T * 64).transpose(2, 3), E


def quant_ref(v, lens):
    B, H, N, D = v.shape
    T = (N + 63) // 64
    valid = (torch.arange(T * 64).view(1, -1) < torch.tensor(lens).view(-1, 1)).view(B, 1, T, 64, 1)
    x = torch.nn.functional.pad(v.double(), (0, 0, 0, T * 64 - N)).view(B, H, T, 64, D)
    x = torch.where(valid, x, torch.zeros((), dtype=torch.float64))               # NaN in invalid rows: never looked at
    half = (torch.arange(64) >> 5).view(1, 1, 1, 64, 1)
    a = torch.stack([(x.abs() * (half == hh)).amax(3) for hh in (0, 1)], 3)       # [B,H,T,2,D]
    m, e = torch.frexp(a)                                                         # a = m 2^e, .5 <= m < 1: a <= 6 * 2^k
    E = torch.where(a == 0, 127, (127 + e - 3 + (m > 0.75)).clamp(0, 254))        # iff k >= e - 3 + (m > .75)
    y = x * torch.exp2(127 - torch.where(half == 0, E[:, :, :, :1], E[:, :, :, 1:]).double())
    lo = ((GRID <= y.abs().unsqueeze(-1)).sum(-1) - 1).clamp(max=7)
    hi = (lo + 1).clamp(max=7)
    dl, dh = y.abs() - GRID[lo], GRID[hi] - y.abs()
    q = GRID[torch.where((dl < dh) | ((dl == dh) & (lo % 2 == 0)), lo, hi)] * torch.sign(y)   # ties: the even code
    return (q * torch.exp2(torch.where(half == 0, E[:, :, :, :1], E[:, :, :, 1:]).double() - 127)).reshape(B, H, T * 64, D), E


def hnd(t, layout):
    return t if layout == "HND" else t.transpose(1, 2)


# ---- 1. the quantizer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dt,layout", itertools.product((64, 128), (torch.float16, torch.bfloat16), ("HND", "NHD")))
def test_quantizer_is_the_rule(D, dt, layout):
    B, H, N, T = 2, 2, 200, 4
    g = torch.Generator().manual_seed(D)
    v = torch.randn(B, H, N, D, generator=g) * torch.exp2(torch.randint(-6, 7, (B, H, T, 1), generator=g).float()
                                                           ).repeat_interleave(64, 2)[:, :, :N]
    v[0, 0, 32:64] = 0                                                            # an all-zero group
    v[1, 0, 70, :] = 65504.0 if dt == torch.float16 else 3.0e38                   # the largest values
    v[1, 1, 64:96, :] = 0                                                         # a group of fp16 subnormals (bf16: tiny values)
    v[1, 1, 64:96:3, :] = 2.0 ** -24 if dt == torch.float16 else 2.0 ** -120
    ties = torch.tensor([6.0, 2.5, 5.0, 0.25, 0.75, 1.25, 1.75, 3.5, -2.5, -5.0, -0.25, 1.0])  # scale 2^e: 6 is the maximum
    v[0, 1, 128:140, :] = ties.view(-1, 1) * 2.0 ** 3
    v[0, 1, 140:192, :] = 0
    v = v.to(dt)
    for lens in ((0, 1), (3, 4), (5, 31), (33, 64), (65, 129), (200, 200)):
        vp = v.clone()
        for b in range(B):
            vp[b, :, lens[b]:] = float("nan")
        ref, E_ref = quant_ref(v, lens)
        img = torch.full((B, H, D, 32 * T), 0xA5, dtype=torch.uint8, device="cuda")
        sc = torch.full((B, H, T, 2 * D), 0xA5, dtype=torch.uint8, device="cuda")
        vg = hnd(vp, layout).contiguous().cuda()
        sa.quant_v_mxfp4(vg, torch.tensor(lens, dtype=torch.int32, device="cuda"), layout, out=(img, sc))
        vg.zero_()  # (no NaN pattern is left behind in memory the allocator hands to later tests)
        got, E = decode(img, sc)
        raw = img.cpu().view(B, H, D, T, 32)
        for b in range(B):
            nt = (lens[b] + 63) // 64
            assert torch.equal(E[b, :, :nt], E_ref[b, :, :nt]), (lens, b)                     # scale bytes, bit for bit
            assert torch.equal(got[b, :, :nt * 64], ref[b, :, :nt * 64]), (lens, b)          # values (-0 == 0)
            # invalid rows decode to 0: no magnitude bit in any of their nibbles; tiles at or beyond nt keep the poison
            assert (got[b, :, lens[b]:nt * 64] == 0).all() and (raw[b, :, :, nt:] == 0xA5).all() and (sc[b, :, nt:].cpu() == 0xA5).all()


# ---- 2. append equals from-scratch -----------------------------------------------------------------------------------------------
# steps of (start_lens, kv_lens) on three batches (the third stays empty): a decode step inside a group, a step across the
# group boundary at row 32, across a tile boundary, a 70-row chunk, start >= len, a rollback of 3 rows
STEPS = [((8, 60, 0), (9, 61, 0)), ((9, 61, 0), (34, 70, 0)), ((34, 70, 0), (104, 140, 0)), ((104, 140, 0), (104, 140, 0)),
         ((104, 140, 0), (101, 137, 0)), ((101, 137, 0), (102, 200, 0))]


@pytest.mark.parametrize("D,gran", [(64, "per_thread"), (128, "per_thread"), (128, "per_warp")])
def test_append_equals_from_scratch(D, gran):
    B, H, N = 3, 2, 200
    g = torch.Generator().manual_seed(7)
    k, v = (torch.randn(B, H, N, D, generator=g).half().cuda() for _ in range(2))
    lens0 = torch.tensor(STEPS[0][0], dtype=torch.int32, device="cuda")
    c4 = sa.SageKVCacheV4.prepare(k, v, lens0, gran)
    ck = sa.SageKVCache.prepare(k, v, lens0, "fp16", gran)
    for start, lens in STEPS:
        for b in range(B):  # the caller writes the new rows (a rollback rewrites nothing)
            if lens[b] > start[b]:
                k[b, :, start[b]:lens[b]] = torch.randn(H, lens[b] - start[b], D, generator=g).half().cuda()
                v[b, :, start[b]:lens[b]] = torch.randn(H, lens[b] - start[b], D, generator=g).half().cuda() * 3
        before = (c4.v4.clone(), c4.v4_scale.clone())
        st, ln = (torch.tensor(x, dtype=torch.int32, device="cuda") for x in (start, lens))
        c4.append(st, ln, 70)
        ck.append(st, ln, 70)
        img, sc = sa.quant_v_mxfp4(v, ln)
        for b in range(B):
            nt = (lens[b] + 63) // 64
            t0 = min(start[b], lens[b] - 1) // 64 if lens[b] else 0
            assert torch.equal(c4.v4[b, :, :, :32 * nt], img[b, :, :, :32 * nt]) and torch.equal(c4.v4_scale[b, :, :nt], sc[b, :, :nt])
            assert torch.equal(c4.v4[b, :, :, :32 * t0], before[0][b, :, :, :32 * t0])       # untouched tiles: no byte changed
            assert torch.equal(c4.v4[b, :, :, 32 * nt:], before[0][b, :, :, 32 * nt:])
            assert torch.equal(c4.v4_scale[b, :, :t0], before[1][b, :, :t0]) and torch.equal(c4.v4_scale[b, :, nt:], before[1][b, :, nt:])
            assert torch.equal(c4.k8[b, :, :lens[b]], ck.k8[b, :, :lens[b]])
            assert torch.equal(c4.k_scale[b, :, :nt * (4 if gran == "per_thread" else 1)],
                               ck.k_scale[b, :, :nt * (4 if gran == "per_thread" else 1)])


# ---- 3. attention against float64 ------------------------------------------------------------------------------------------------
_CACHES = {}


def _case(D, gran, N):
    """one prepared cache (and its FP8 twin, and V') per (D, gran, N), shared by the cases that attend it"""
    if (D, gran, N) not in _CACHES:
        g = torch.Generator().manual_seed(N + D)
        lens = (0, 1, 128, 200) if N == 200 else (0, 1, 1024, 1100)
        k, v = (torch.randn(4, 1, N, D, generator=g).half() for _ in range(2))
        ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
        c4 = sa.SageKVCacheV4.prepare(k.cuda(), v.cuda(), ln, gran)
        c8 = sa.SageKVCache.prepare(k.cuda(), v.cuda(), ln, "fp8", gran)
        _CACHES[D, gran, N] = (lens, ln, k, c4, c8, decode(c4.v4, c4.v4_scale)[0], c4.km.cpu())
    return _CACHES[D, gran, N]


ATTN = [(D, gran, M, N, S, fold) for D, gran, M, N, S, fold in itertools.product(
    (64, 128), ("per_thread", "per_warp"), (1, 4, 16, 130), (200, 1100), (1, 2, 3), (0, 1, 4)) if fold == 0 or M % fold == 0]


@pytest.mark.parametrize("D,gran,M,N,S,fold", ATTN)
def test_attention_against_float64(D, gran, M, N, S, fold):
    """|o - W V'| <= min(2^-4 W|V'|, 6 sqrt(2^-8/3 W^2 V'^2)) + 2 ulps max(|o_ref|, .25) on EVERY element: one e4m3 rounding
    of P (half an ulp of 3 mantissa bits, relative 2^-4; variance 2^-8/3 of a uniform relative error in +-2^-4) against the
    unrounded reference, the products with the FP4 values and the block scales exact in the MFMA; lse bit-equal to the FP8
    cache's."""
    lens, ln, k, c4, c8, vprime, km = _case(D, gran, N)
    Hq = 2
    q = torch.randn(4, Hq, M, D, generator=torch.Generator().manual_seed(M)).half()
    causal = fold > 0
    o, lse = sa.sageattn_splitkv_v4(q.cuda(), c4, ln, S, causal, max(fold, 1), return_lse=True)
    _, lse8 = sa.sageattn_splitkv_cached(q.cuda(), c8, ln, S, causal, max(fold, 1), return_lse=True)
    assert torch.equal(lse, lse8)
    o, lse = o.cpu().double(), lse.cpu()
    quant = O.per_thread_int8 if gran == "per_thread" else O.per_warp_int8
    worst = 0.0
    for b, n in enumerate(lens):
        keep = allowed_keys(n, M, fold, n) if causal else torch.ones(M, n, dtype=torch.bool)
        rows = keep.any(1)
        assert (o[b][:, ~rows] == 0).all() and (lse[b][:, ~rows] == float("-inf")).all()    # rows without keys
        if n == 0:
            continue
        q8, qs, k8, ks = quant(q[b:b + 1], k[b:b + 1, :, :n], km[b:b + 1].unsqueeze(2))
        W = softmax_weights(q8, k8, O.expand_q_scale(qs, M, gran), O.expand_k_scale(ks, n, gran), D ** -0.5 * 1.44269504)
        W = W[0].double() * keep
        W = W / W.sum(-1, keepdim=True).clamp(min=1e-300)
        V = vprime[b, :, :n]                                                                # [1, n, D]: the cache's own image
        ref = W @ V
        bound = torch.minimum(2.0 ** -4 * (W @ V.abs()), 6 * torch.sqrt((2.0 ** -8 / 3) * ((W * W) @ (V * V)))) \
            + 2 * 2.0 ** -10 * ref.abs().clamp(min=0.25)
        ratio = ((o[b] - ref).abs() / bound)[:, rows].max().item() if rows.any() else 0.0
        print(f"b={b} len={n}: max |o - ref| / bound = {ratio:.3f}")
        worst = max(worst, ratio)
    assert worst <= 1.0, worst


# ---- 4. graph and compile ----------------------------------------------------------------------------------------------------------
def _step_tensors():
    g = torch.Generator().manual_seed(3)
    k, v = (torch.randn(2, 2, 320, 128, generator=g).half().cuda() for _ in range(2))
    q = torch.randn(2, 4, 4, 128, generator=g).half().cuda()
    lens = torch.tensor([190, 63], dtype=torch.int32, device="cuda")
    return q, k, v, lens


def test_graph_replay_equals_eager():
    q, k, v, lens = _step_tensors()
    cache, eager = sa.SageKVCacheV4.prepare(k, v, lens), sa.SageKVCacheV4.prepare(k, v, lens)
    start = lens.clone()

    def step(c):
        c.append(start, lens, 1)
        return sa.sageattn_splitkv_v4(q, c, lens, 2, True, 4)

    step(cache)  # warm-up outside the capture (workspace and library state)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(cache)
    for _ in range(3):  # kv_lens grows by one per replay; the replay reads the lengths the tensors hold then
        start.copy_(lens)
        lens.add_(1)
        graph.replay()
        assert torch.equal(out, step(eager))
        assert torch.equal(cache.v4, eager.v4) and torch.equal(cache.v4_scale, eager.v4_scale)


def test_compile_fullgraph_equals_eager():
    q, k, v, lens = _step_tensors()
    cache, eager = sa.SageKVCacheV4.prepare(k, v, lens), sa.SageKVCacheV4.prepare(k, v, lens)
    ops = torch.ops.sageattention_amd_fp4

    def step(q, k, v, km, k8, ks, v4, v4s, start, lens):
        ops.kv_cache_append_v4(k, v, km, k8, ks, v4, v4s, start, lens, 1, "HND", "per_thread")
        return ops.attn_splitkv_v4_lse(q, k8, ks, km, v4, v4s, lens, 2, "HND", 128 ** -0.5, "per_thread")

    args = lambda c: (q, k, v, c.km, c.k8, c.k_scale, c.v4, c.v4_scale, lens - 1, lens)  # noqa: E731
    o, lse = torch.compile(step, fullgraph=True)(*args(cache))
    o_e, lse_e = step(*args(eager))
    assert torch.equal(o, o_e) and torch.equal(lse, lse_e) and torch.equal(cache.v4, eager.v4)
