"""The paged cache without fp16 pools (``SagePagedRowCache``, include/sageattn_hip_paged_rows.h) without a GPU: the header
against its ctypes table, the C status table of the entry point, the Python refusals, the torch.library op and its fake, and the
model of the ring of two tile slots.  What the kernel computes: test_paged_rows_gpu.py."""
import ctypes
import os
import random
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import paged_rows_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = "sageattention_amd_paged_rows"
ENTRY = "sage_kv_cache_append_rows_paged"


# ---- 1. the header against its table -----------------------------------------------------------------------------------------
def _prototypes(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    ctype = lambda s: re.sub(r"\bconst\b|\s", "", s)  # noqa: E731
    out = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\s*\b(sage_\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = (ctype(ret), [ctype(re.sub(r"\w+$", "", p.strip())) for p in params.split(",")])
    return out


def test_header_matches_its_table():
    from sageattention_amd import _lib as L
    protos = _prototypes("sageattn_hip_paged_rows.h")
    assert list(protos) == list(L.PAGED_ROWS_SIGNATURES) == [ENTRY]
    want = {"int": ctypes.c_int, "sage_stream_t": ctypes.c_void_p, "int64_t": ctypes.c_int64}
    ret, params = protos[ENTRY]
    res, args = L.PAGED_ROWS_SIGNATURES[ENTRY]
    assert res is want[ret] and len(params) == len(args) == 24
    for c, ct in zip(params, args):
        if c == "sage_tensor*":
            assert ct is ctypes.POINTER(L.SageTensor), c
        elif c.endswith("*"):
            assert c[:-1] in ("void", "float", "int32_t") and ct is ctypes.c_void_p, c
        else:
            assert ct is want[c], c
    # the other headers and their tables are what they were
    assert len(L.SIGNATURES) == 69 and list(L.KVCACHE_SIGNATURES) == ["sage_kv_cache_append"] and len(L.PAGED_SIGNATURES) == 3
    assert ENTRY not in {**L.SIGNATURES, **L.KVCACHE_SIGNATURES, **L.PAGED_SIGNATURES}
    for header in ("sageattn_hip.h", "sageattn_hip_kvcache.h", "sageattn_hip_paged.h"):
        assert "_rows_paged(" not in open(os.path.join(ROOT, "include", header)).read()
    assert L.lib().sage_abi_version() == 3


def test_symbol_exported_and_bound():
    from sageattention_amd import _lib as L
    fn = getattr(L.lib(), ENTRY)
    assert fn.restype is ctypes.c_int and fn.argtypes == L.PAGED_ROWS_SIGNATURES[ENTRY][1]


# ---- 2. the C status table ---------------------------------------------------------------------------------------------------------
# Fake device addresses: where a GPU is visible a missed check would launch the kernel on them, so this runs only where none
# is; there every launch attempt returns SAGE_ERR_LAUNCH (-5), which makes a launch observable (tests/test_cabi_symbols.py).
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")
FAKE = 1 << 20
_ARGS = ("k_new v_new dt B H T D km tail k8 ks gran rnd v_pool v8 coef table tstride max_pages page_size P start lens stream")


def _pool(stride_n=64, data=FAKE):
    from sageattention_amd import _lib as L
    return L.SageTensor(data, 1 << 16, 1 << 13, stride_n)


def _rows(data=FAKE, stride_n=64):
    from sageattention_amd import _lib as L
    return L.SageTensor(data, 1 << 12, 1 << 10, stride_n)


def _call(**change):
    from sageattention_amd import _lib as L
    args = dict(k_new=_rows(), v_new=_rows(), dt=0, B=2, H=2, T=3, D=64, km=FAKE, tail=FAKE, k8=_pool(), ks=FAKE, gran=3, rnd=0,
                v_pool=None, v8=_pool(128), coef=FAKE, table=FAKE, tstride=5, max_pages=5, page_size=128, P=24, start=FAKE,
                lens=FAKE, stream=None)
    args.update(change)
    return L.lib().sage_kv_cache_append_rows_paged(*[args[n] for n in _ARGS.split()])


def _f16():
    return dict(v_pool=_pool(), v8=None, coef=None)


@no_gpu
def test_valid_calls_reach_a_launch():
    assert _call() == -5
    assert _call(**_f16()) == -5
    assert _call(**dict(_f16(), coef=FAKE + 4)) == -5                    # v_coef is not read without v8_pool
    for ps in (64, 128, 256):
        assert _call(page_size=ps, v8=_pool(ps)) == -5
    assert _call(T=1) == -5 and _call(T=4096) == -5
    assert _call(tstride=9, max_pages=1, P=1, gran=1, rnd=1, dt=1, D=128, table=FAKE + 4) == -5
    # a strided view of a fused projection: strides that are multiples of 16 bytes
    assert _call(k_new=_rows(FAKE + 128, 3 * 64), v_new=_rows(FAKE + 256, 3 * 64)) == -5
    from sageattention_amd import _lib as L
    assert _call(k8=L.SageTensor(FAKE, 1 << 40, 1 << 13, 64)) == -5  # a page slice that fits is addressed wherever the page lies


@no_gpu
def test_status_table():
    """Each argument made invalid on its own returns its argument status -- the one the paged append gives the same fault --:
    nothing was launched (a launch returns -5 here)."""
    from sageattention_amd import _lib as L
    odd = L.SageTensor(FAKE + 8, 1 << 16, 1 << 13, 64)
    far = L.SageTensor(FAKE, 1 << 40, 1 << 36, 1 << 26)   # a (page, head) slice of 128 rows x 2^26 bytes: beyond the window
    cases = [
        (dict(page_size=32), -1), (dict(page_size=16), -1), (dict(page_size=96), -1), (dict(page_size=512), -1),
        (dict(page_size=0), -1), (dict(table=None), -1), (dict(table=FAKE + 2), -1), (dict(table=FAKE + 1), -1),
        (dict(max_pages=0), -1), (dict(max_pages=-1), -1), (dict(P=0), -1), (dict(P=-3), -1), (dict(tstride=4), -1),
        (dict(tstride=0), -1), (dict(max_pages=1 << 24, tstride=1 << 24, page_size=256), -4),
        (dict(k_new=None), -1), (dict(v_new=None), -1), (dict(k8=None), -1), (dict(km=None), -1), (dict(ks=None), -1),
        (dict(start=None), -1), (dict(lens=None), -1), (dict(km=FAKE + 8), -1), (dict(coef=FAKE + 8), -1),
        (dict(start=FAKE + 2), -1), (dict(lens=FAKE + 1), -1), (dict(k_new=_rows(FAKE + 8)), -1), (dict(v_new=_rows(FAKE + 8)), -1),
        (dict(k_new=_rows(FAKE, 68)), -1), (dict(v_new=_rows(FAKE, 68)), -1), (dict(k8=odd), -1), (dict(v8=odd), -1),
        (dict(coef=None), -1), (dict(D=96), -2), (dict(D=32), -2), (dict(D=256), -2), (dict(gran=2), -1), (dict(gran=0), -1),
        (dict(gran=4), -1), (dict(rnd=2), -1), (dict(dt=2), -1), (dict(B=0), -1), (dict(H=0), -1),
        # the entry point's own
        (dict(T=0), -1), (dict(T=-1), -1), (dict(tail=None), -1), (dict(tail=FAKE + 8), -1), (dict(tail=FAKE + 2), -1),
        (dict(v8=None), -1), (dict(v8=None, coef=None), -1), (dict(v_pool=_pool()), -1),          # neither, both
        (dict(v_pool=odd, v8=None, coef=None), -1), (dict(k8=far), -4), (dict(v8=far), -4), (dict(v_pool=far, v8=None, coef=None), -4)]
    wrong = [(sorted(c), st, got) for c, st in cases if (got := _call(**c)) != st]
    assert not wrong, wrong


# ---- 3. Python refusals, raised before any device call ---------------------------------------------------------------------------
def _cpu_cache(pv="fp16", D=64, layout="HND", page_size=128, P=6, B=2, dtype=torch.float16):
    import sageattention_amd as sa
    return sa.SagePagedRowCache.allocate(P, page_size, B, 2, D, dtype, "cpu", pv=pv, tensor_layout=layout)


def test_allocate_state_and_refusals():
    import sageattention_amd as sa
    from sageattention_amd import paged_rows
    assert "SagePagedRowCache" in sa.__all__ and sa.SagePagedRowCache is paged_rows.SagePagedRowCache
    A = sa.SagePagedRowCache.allocate
    c = A(6, 128, 2, 2, 64, torch.float16, "cpu", pv="fp8")
    assert c.k8.shape == (6, 2, 128, 64) and c.k8.dtype == torch.int8 and c.k_scale.shape == (6, 2, 8)
    assert c.k_tail.shape == (2, 2, 2, 64, 64) and c.k_tail.dtype == torch.float16 and c.km.shape == (2, 2, 64)
    assert c.v8.shape == (6, 2, 64, 128) and c.v8.dtype == torch.float8_e4m3fn and c.v_pool is None and c.v is c.v8
    assert c.v_scale.shape == (2, 2, 64) and c.v_coef.shape == (2, 2, 2, 64)
    assert not hasattr(c, "k")                                     # there is no fp16 K pool anywhere
    c = A(6, 64, 3, 2, 128, torch.bfloat16, "cpu", pv="fp16", qk_quant_gran="per_warp", tensor_layout="NHD")
    assert c.k8.shape == (6, 64, 2, 128) and c.k_scale.shape == (6, 2, 1) and c.v8 is None and c.v_scale is None
    assert c.v_pool.shape == c.k8.shape and c.v_pool.dtype == torch.bfloat16 and c.v is c.v_pool
    # nbytes: all state.  Per cached key and KV head at head_dim 128: 256.25 (FP8 P.V), 384.25 (FP16 P.V), plus the rest
    P, ps, B, Hk, D = 16, 128, 2, 2, 128
    per_seq = B * Hk * (2 * 64 * D * 2 + D * 2)                     # the tail and km
    assert A(P, ps, B, Hk, D, torch.float16, "cpu", pv="fp16").nbytes() == int(P * ps * Hk * 384.25) + per_seq
    assert A(P, ps, B, Hk, D, torch.float16, "cpu", pv="fp8").nbytes() == int(P * ps * Hk * 256.25) + per_seq + B * Hk * D * 12
    for bad in (32, 16, 96, 320, 512):
        with pytest.raises(ValueError, match="page_size must be 64, 128 or 256.*64-key tiles"):
            A(6, bad, 2, 2, 64, torch.float16, "cpu")
    for bad in (72, 32, 256):
        with pytest.raises(ValueError, match="head_dim 64 or 128"):
            A(6, 128, 2, 2, bad, torch.float16, "cpu")
    with pytest.raises(ValueError, match="dtype"):
        A(6, 128, 2, 2, 64, torch.float32, "cpu")
    with pytest.raises(ValueError, match="pv"):
        A(6, 128, 2, 2, 64, torch.float16, "cpu", pv="int8")
    with pytest.raises(ValueError, match="qk_quant_gran"):
        A(6, 128, 2, 2, 64, torch.float16, "cpu", qk_quant_gran="per_block")
    with pytest.raises(ValueError, match="layout"):
        A(6, 128, 2, 2, 64, torch.float16, "cpu", tensor_layout="BHSD")
    with pytest.raises(TypeError, match="v_headroom"):
        A(6, 128, 2, 2, 64, torch.float16, "cpu", v_headroom="2")
    for bad in (0.5, 0, float("nan")):
        with pytest.raises(ValueError, match="v_headroom"):
            A(6, 128, 2, 2, 64, torch.float16, "cpu", v_headroom=bad)
    with pytest.raises(ValueError, match=">= 1"):
        A(0, 128, 2, 2, 64, torch.float16, "cpu")
    with pytest.raises(TypeError, match="num_pages"):
        A(6.0, 128, 2, 2, 64, torch.float16, "cpu")


def _table_refusals(call, B=2):
    with pytest.raises(TypeError, match="block_table"):
        call([[0, 1, 2]] * B)
    with pytest.raises(TypeError, match="block_table must be of dtype int32"):
        call(torch.zeros(B, 3, dtype=torch.int64))
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(B, 3, 1, dtype=torch.int32), torch.zeros(B, 0, dtype=torch.int32),
                torch.zeros(B + 1, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="block_table shape"):
            call(bad)
    with pytest.raises(ValueError, match="block_table is on"):
        call(torch.zeros(B, 3, dtype=torch.int32, device="meta"))
    with pytest.raises(ValueError, match=r"stride\(-1\) == 1"):
        call(torch.zeros(B, 6, dtype=torch.int32)[:, ::2])


@pytest.mark.parametrize("method", ["append_rows", "prepare_"])
def test_rows_refusals(method):
    cache = _cpu_cache()
    table = torch.zeros(2, 3, dtype=torch.int32)
    lens = torch.tensor([80, 3], dtype=torch.int32)
    k = torch.zeros(2, 2, 5, 64, dtype=torch.float16)
    if method == "append_rows":
        f = lambda k_, v_, t=table, s=lens, n=lens: cache.append_rows(k_, v_, t, s, n)  # noqa: E731
    else:
        f = lambda k_, v_, t=table, s=lens, n=lens: cache.prepare_(k_, v_, t, n)  # noqa: E731
    with pytest.raises(TypeError, match="must be tensors"):
        f(k, None)
    with pytest.raises(ValueError, match="4-D"):
        f(k[0], k[0])
    with pytest.raises(ValueError, match="one shape"):
        f(k, k[:, :, :4])
    with pytest.raises(ValueError, match="one shape"):
        f(k, k[:, :1])
    with pytest.raises(ValueError, match="dtype"):
        f(k.bfloat16(), k.bfloat16())
    with pytest.raises(ValueError, match="dtype"):
        f(k, k.float())
    with pytest.raises(ValueError, match="the cache on"):
        f(k, k.to("meta"))
    for bad in (torch.zeros(3, 2, 5, 64), torch.zeros(2, 4, 5, 64), torch.zeros(2, 2, 5, 128), torch.zeros(2, 2, 0, 64),
                torch.zeros(2, 5, 2, 64)):                                # (the last: NHD rows for an HND cache)
        with pytest.raises(ValueError, match="does not match"):
            f(bad.half(), bad.half())
    with pytest.raises(ValueError, match=r"stride\(-1\) == 1"):
        f(torch.zeros(2, 2, 5, 128, dtype=torch.float16)[..., ::2], k)
    _table_refusals(lambda t: f(k, k, t=t))
    with pytest.raises(TypeError, match="int32"):
        f(k, k, n=lens.long())
    with pytest.raises(TypeError, match="kv_lens"):
        f(k, k, n=[80, 3])
    with pytest.raises(ValueError, match="kv_lens shape"):
        f(k, k, n=torch.zeros(3, dtype=torch.int32))
    if method == "append_rows":
        with pytest.raises(TypeError, match="int32"):
            f(k, k, s=lens.long())
        with pytest.raises(ValueError, match="is on"):
            f(k, k, s=lens.to("meta"))
    else:   # a prompt beyond the capacity of the table: 3 pages of 128
        big = torch.zeros(2, 2, 385, 64, dtype=torch.float16)
        with pytest.raises(ValueError, match="capacity of 384"):
            f(big, big)


def test_attention_accepts_the_cache_and_refuses_as_before():
    """``sageattn_splitkv_paged`` reads dtype, head_dim and Hk from either cache: the refusals of test_paged.py in the same words"""
    import sageattention_amd as sa
    cache = _cpu_cache()
    q = torch.zeros(2, 4, 8, 64, dtype=torch.float16)
    table = torch.zeros(2, 3, dtype=torch.int32)
    lens = torch.tensor([80, 3], dtype=torch.int32)
    f = sa.sageattn_splitkv_paged
    k = torch.zeros(6, 2, 128, 64, dtype=torch.float16)
    bound = sa.SagePagedKVCache(k, k.clone(), "fp16", "per_thread", "HND", 2.0)
    bound.km = torch.zeros(2, 2, 64, dtype=torch.float16)
    for kw in (dict(is_causal=True), dict(attn_mask=torch.ones(8, 320, dtype=torch.bool)), dict(smooth_k=False)):
        with pytest.raises(ValueError, match="does not take") as e:
            f(q, cache, table, lens, 2, **kw)
        with pytest.raises(ValueError) as e2:
            f(q, bound, table, lens, 2, **kw)
        assert str(e.value) == str(e2.value)
    with pytest.raises(TypeError, match="cache must be a SagePagedKVCache"):
        f(q, object(), table, lens)
    _table_refusals(lambda t: f(q, cache, t, lens))
    with pytest.raises(TypeError, match="kv_lens"):
        f(q, cache, table, None)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="num_splits"):
            f(q, cache, table, lens, bad)
    with pytest.raises(ValueError, match="q_fold"):
        f(q, cache, table, lens, causal=False, q_fold=2)
    for call_cache in (cache, bound):
        with pytest.raises(ValueError, match="head_dim 64, got 128"):
            f(torch.zeros(2, 4, 8, 128, dtype=torch.float16), call_cache, table, lens)
        with pytest.raises(ValueError, match="dtype and device of the cache's k"):
            f(q.bfloat16(), call_cache, table, lens)
        with pytest.raises(ValueError, match=r"num_qo_heads \(3\) must be divisible by num_kv_heads \(2\)"):
            f(torch.zeros(2, 3, 8, 64, dtype=torch.float16), call_cache, table, lens, 2)
        with pytest.raises(ValueError, match="q has 1 sequences, the cache 2"):
            f(q[:1], call_cache, table[:1], lens[:1], 2)


# ---- 4. the torch.library op ---------------------------------------------------------------------------------------------------------
def test_op_lives_in_its_own_namespace():
    import sageattention_amd  # noqa: F401
    import sageattention_amd.ops  # noqa: F401
    names = torch._C._dispatch_get_all_op_names()
    assert [n.split("::")[1] for n in names if n.startswith(NS + "::")] == ["kv_cache_append_rows_paged"]
    assert len([n for n in names if n.startswith("sageattention_amd::")]) == 26
    assert len([n for n in names if n.startswith("sageattention_amd_kvcache::")]) == 5
    assert len([n for n in names if n.startswith("sageattention_amd_paged::")]) == 5
    s = str(getattr(torch.ops, NS).kv_cache_append_rows_paged.default._schema)
    assert s.endswith("-> ()")
    for name in ("k_tail", "k8", "k_scale"):
        assert re.search(rf"Tensor\(\w+!\) {name}\b", s), (name, s)
    for name in ("v_pool", "v8"):
        assert re.search(rf"Tensor\(\w+!\)\? {name}\b", s), (name, s)
    assert not re.search(r"Tensor\(\w+!\)\??\s+(k_new|v_new|km|v_coef|block_table|start_lens|kv_lens)\b", s), s
    assert "Tensor k_new, Tensor v_new, Tensor km" in s and "Tensor block_table, Tensor start_lens, Tensor kv_lens" in s
    assert "max_new" not in s                                       # the grid follows T = k_new.size(-2)


@pytest.mark.parametrize("layout", ["HND", "NHD"])
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_fake(layout, pv):
    """the append returns nothing, attention on the cache describes its outputs, ``narrow`` shares the pools"""
    import sageattention_amd as sa
    with FakeTensorMode():
        D, B, HQ, HK, M, P, ps = 128, 2, 4, 2, 8, 7, 128
        cache = sa.SagePagedRowCache.allocate(P, ps, B, HK, D, torch.bfloat16, "cuda", pv=pv, qk_quant_gran="per_warp",
                                              tensor_layout=layout)
        lens = torch.empty((B,), dtype=torch.int32, device="cuda")
        table = torch.empty((B, 3), dtype=torch.int32, device="cuda")
        rows = torch.empty((B, HK, 5, D) if layout == "HND" else (B, 5, HK, D), dtype=torch.bfloat16, device="cuda")
        assert cache.append_rows(rows, rows, table, lens, lens) is None
        fused = torch.empty((B, 5, 3 * HK * D), dtype=torch.bfloat16, device="cuda").view(B, 5, 3, HK, D)
        k_view = fused[:, :, 1] if layout == "NHD" else fused[:, :, 1].transpose(1, 2)
        assert cache.append_rows(k_view, k_view, table, lens, lens) is None
        qshape = (B, HQ, M, D) if layout == "HND" else (B, M, HQ, D)
        q = torch.empty(qshape, dtype=torch.bfloat16, device="cuda")
        o, lse = sa.sageattn_splitkv_paged(q, cache, table, lens, 3, return_lse=True, causal=True, q_fold=2)
        assert o.shape == q.shape and o.dtype == q.dtype and o.is_contiguous()
        assert lse.shape == (B, HQ, M) and lse.dtype == torch.float32
        c1 = cache.narrow(1, 1)
        assert c1.km.shape[0] == c1.k_tail.shape[0] == 1 and c1.k8 is cache.k8 and c1.k_scale is cache.k_scale
        assert c1.v8 is cache.v8 and c1.v_pool is cache.v_pool and c1.page_size == ps and c1.dtype == torch.bfloat16
        assert (pv == "fp16" and c1.v_scale is None) or c1.v_scale.shape[0] == c1.v_coef.shape[0] == 1
        assert c1.nbytes() < cache.nbytes()


# ---- 5. the ring of two tile slots ---------------------------------------------------------------------------------------------------
def test_ring_homes_and_geometry():
    assert RU.ring_home(0) == (0, 0) and RU.ring_home(63) == (0, 63) and RU.ring_home(64) == (1, 0) and RU.ring_home(130) == (0, 2)
    assert RU.call_geometry(5, 0) is None and RU.call_geometry(-3, 600) == (0, 512, 512, 0, 0, 7)
    assert RU.call_geometry(66, 63) == (66, 63, 0, 63, 0, 0)                # a rollback: the tile of row 62 alone
    assert list(RU.ring_read_rows(66, 63)) == list(range(0, 63)) and list(RU.ring_written_rows(66, 63)) == []
    assert list(RU.ring_read_rows(60, 130)) == list(range(0, 60))           # the hazard: tile 0 is read from slot 0 ...
    assert list(RU.ring_written_rows(60, 130)) == list(range(64, 130))      # ... and the rows of tile 2 go to slot 0
    assert {RU.ring_home(r)[0] for r in range(128, 130)} == {0}
    assert list(RU.ring_written_rows(0, 512)) == list(range(384, 512)) and list(RU.ring_read_rows(0, 512)) == []
    assert sorted(RU.token_of_pos(p) for p in range(64)) == list(range(64))
    assert [RU.token_of_pos(p) for p in (0, 1, 2, 3, 4, 16, 32)] == [0, 1, 2, 3, 8, 32, 4]


def test_ring_serves_every_admitted_call_after_a_first_one():
    """exhaustive over a 512-key capacity: every (old length, s, len) that meets the precondition reads the rows it expects
    (all 513^3 triples, vectorised per old length), and the scalar model agrees on the boundary cases of every old length"""
    admitted_total = 0
    for old in range(RU.CAP + 1):
        admitted, served = RU.first_call_grid(old)
        assert bool((served | ~admitted).all()), old
        admitted_total += int(admitted.sum())
        hi = (old - 1) >> 6 if old else -1
        for s, ln in {(old, old + 1), (old, old + 70), (old, RU.CAP), (old, old), (max(old - 1, 0), old), (max(old - 64, 0), old),
                      (max(old - 64, 0), max(old - 64, 0)), (max(64 * (hi - 1), 0), RU.CAP), (old + 5, max(64 * (hi - 1), 0) + 1)}:
            ln = min(ln, RU.CAP)
            m = RU.RingModel()
            assert m.append(0, old) == [] and m.hi == hi
            assert bool(admitted[min(s, RU.CAP), ln]) == m.admitted(s, ln), (old, s, ln)
            if m.admitted(s, ln):
                assert m.append(s, ln) == [], (old, s, ln)
                assert m.append(ln, ln) == [], (old, s, ln)          # and the ring then serves the ragged tile again
    assert admitted_total > 10_000_000                               # (the walk is not vacuous)


@pytest.mark.parametrize("seed", range(8))
def test_ring_serves_random_admitted_sequences(seed):
    """200 admitted calls: decode steps, chunks of up to 200 rows, rollbacks of up to 64 rows, overwrite-and-extend, and a
    fresh prepare when the capacity is reached; every ring read finds the id it expects"""
    rng = random.Random(seed)
    m = RU.RingModel()
    steps = 0
    seen = set()
    assert m.append(0, rng.randrange(0, 200)) == []
    while steps < 200:
        old = len(m.rows)
        kind = rng.choice(["step", "step", "chunk", "rollback", "overwrite", "again"])
        if old >= RU.CAP - 1 or old == 0:                        # full, or rolled back to nothing: the slot is prepared again
            m, kind = RU.RingModel(), "prepare"
            s, ln = 0, rng.randrange(0, 300)
        elif kind == "step":
            s, ln = old, old + 1
        elif kind == "chunk":
            s, ln = old, min(old + rng.randrange(2, 201), RU.CAP)
        elif kind == "rollback":
            ln = max(old - rng.randrange(1, 65), 0)
            s = rng.choice([ln, old])                                # start == len, or start >= len
        elif kind == "overwrite":
            s = max(old - rng.randrange(1, 65), 0)
            ln = min(old + rng.randrange(0, 70), RU.CAP)
        else:
            s, ln = old, old
        if not m.admitted(s, ln):
            continue
        assert m.append(s, ln) == [], (seed, steps, kind, old, s, ln)
        assert len(m.rows) == ln
        steps += 1
        seen.add(kind)
    assert {"step", "chunk", "rollback", "overwrite", "again"} <= seen


def test_a_call_outside_the_precondition_reads_a_stale_row():
    """why the precondition exists: two tile boundaries back, the slot of the tile holds the rows of the tile two above it"""
    m = RU.RingModel()
    assert m.append(0, 130) == [] and m.hi == 2
    assert not m.admitted(63, 63)                                    # t0 = 0 < hi - 1 = 1
    wrong = m.append(63, 63)
    assert [w[0] for w in wrong] == list(range(63)) and [w[1] for w in wrong] == list(range(63))
    assert [w[2] for w in wrong[:2]] == [128, 129]                   # rows 0 and 1 of slot 0 are rows 128 and 129 ...
    assert all(w[2] is None for w in wrong[2:])                      # ... and the call from 0 to 130 never wrote the others
    # one boundary back is admitted: 130 -> 100 -> 66, never past two
    m = RU.RingModel()
    assert m.append(0, 130) == [] and m.admitted(100, 100) and m.append(100, 100) == []
    assert m.admitted(66, 66) and m.append(66, 66) == [] and not m.admitted(63, 63)
