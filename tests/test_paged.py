"""The paged KV cache (``SagePagedKVCache``, ``sageattn_splitkv_paged``, include/sageattn_hip_paged.h) without a GPU: the new
header against its ctypes table, the C status table of the three entry points, the Python refusals, the torch.library ops and
the tile-to-page arithmetic.  What the kernels compute: test_paged_gpu.py."""
import ctypes
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import kvcache_util as KU
import paged_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = "sageattention_amd_paged"
OPS = ("kv_cache_append_paged", "attn_splitkv_paged", "attn_splitkv_paged_lse", "attn_splitkv_causal_paged",
       "attn_splitkv_causal_paged_lse")
ENTRIES = ("sage_kv_cache_append_paged", "sage_attn_fusedq_pv_f16_splitkv_paged", "sage_attn_fusedq_pv_f8_splitkv_paged")


# ---- 1. the new header against its table -----------------------------------------------------------------------------------------
def _prototypes(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    ctype = lambda s: re.sub(r"\bconst\b|\s", "", s)  # noqa: E731
    out = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\s*\b(sage_\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = (ctype(ret), [ctype(re.sub(r"\w+$", "", p.strip())) for p in params.split(",")])
    return out


def test_paged_header_matches_its_table():
    from sageattention_amd import _lib as L
    protos = _prototypes("sageattn_hip_paged.h")
    assert sorted(protos) == sorted(L.PAGED_SIGNATURES) == sorted(ENTRIES)
    want = {"int": ctypes.c_int, "sage_stream_t": ctypes.c_void_p, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float}
    for name, (ret, params) in protos.items():
        res, args = L.PAGED_SIGNATURES[name]
        assert res is want[ret] and len(params) == len(args) == (22 if name == ENTRIES[0] else 30), name
        for c, ct in zip(params, args):
            if c == "sage_tensor*":
                assert ct is ctypes.POINTER(L.SageTensor), (name, c)
            elif c.endswith("*"):
                assert c[:-1] in ("void", "float", "int32_t") and ct is ctypes.c_void_p, (name, c)
            else:
                assert ct is want[c], (name, c)
    # the other headers and their tables are what they were
    assert len(L.SIGNATURES) == 69 and list(L.KVCACHE_SIGNATURES) == ["sage_kv_cache_append"]
    assert not set(L.PAGED_SIGNATURES) & (set(L.SIGNATURES) | set(L.KVCACHE_SIGNATURES))
    for header in ("sageattn_hip.h", "sageattn_hip_kvcache.h"):
        assert "_paged(" not in open(os.path.join(ROOT, "include", header)).read()
    assert L.lib().sage_abi_version() == 3


def test_symbols_exported_and_bound():
    from sageattention_amd import _lib as L
    for name in ENTRIES:
        fn = getattr(L.lib(), name)
        assert fn.restype is ctypes.c_int and fn.argtypes == L.PAGED_SIGNATURES[name][1]


# ---- 2. the C status table ---------------------------------------------------------------------------------------------------------
# Fake device addresses: where a GPU is visible a missed check would launch kernels on them, so this runs only where none
# is; there every launch attempt returns SAGE_ERR_LAUNCH (-5), which makes a launch observable (tests/test_cabi_symbols.py).
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")
FAKE = 1 << 20
_APPEND = "k v dt B H D km k8 ks gran rnd v8 coef table tstride max_pages page_size P start lens max_new stream"
_ATTN_TAIL = "B Hq Hk M D gran warpq sm_scale table tstride max_pages page_size P lens num_splits causal q_fold ws ws_bytes stream"
_ATTN = {"f16": "q q_dt k8 v v_dt o o_dt ks km lse " + _ATTN_TAIL, "f8": "q q_dt k8 v o o_dt ks km v_scale lse " + _ATTN_TAIL}


def _pool(stride_n=64, data=FAKE):
    from sageattention_amd import _lib as L
    return L.SageTensor(data, 1 << 16, 1 << 13, stride_n)


def _append(**change):
    from sageattention_amd import _lib as L
    args = dict(k=_pool(), v=_pool(), dt=0, B=2, H=2, D=64, km=FAKE, k8=_pool(), ks=FAKE, gran=3, rnd=0, v8=_pool(128),
                coef=FAKE, table=FAKE, tstride=5, max_pages=5, page_size=128, P=24, start=FAKE, lens=FAKE, max_new=1, stream=None)
    args.update(change)
    return L.lib().sage_kv_cache_append_paged(*[args[n] for n in _APPEND.split()])


def _attn(pv, **change):
    from sageattention_amd import _lib as L
    t = L.SageTensor(FAKE, 1 << 16, 1 << 12, 64)
    args = dict(q=t, q_dt=0, k8=_pool(), v=_pool(128 if pv == "f8" else 64), v_dt=0, o=t, o_dt=0, ks=FAKE, km=FAKE, v_scale=FAKE,
                lse=None, B=2, Hq=4, Hk=2, M=8, D=64, gran=3, warpq=32, sm_scale=0.125, table=FAKE, tstride=5, max_pages=5,
                page_size=128, P=24, lens=FAKE, num_splits=2, causal=0, q_fold=1, ws=FAKE, ws_bytes=1 << 30, stream=None)
    args.update(change)
    return getattr(L.lib(), f"sage_attn_fusedq_pv_{pv}_splitkv_paged")(*[args[n] for n in _ATTN[pv].split()])


@no_gpu
def test_valid_calls_reach_a_launch():
    assert _append() == -5
    assert _append(v=None, v8=None, coef=None) == -5
    for ps in (64, 128, 256):
        assert _append(page_size=ps, v8=_pool(ps)) == -5
    assert _append(tstride=9, max_pages=1, P=1, gran=1, rnd=1, dt=1, D=128, table=FAKE + 4) == -5
    for pv in ("f16", "f8"):
        assert _attn(pv) == -5
        assert _attn(pv, causal=1, q_fold=4, lse=FAKE, num_splits=1, page_size=64, tstride=7, table=FAKE + 4) == -5
        assert _attn(pv, causal=0, q_fold=0) == -5          # q_fold is not read without causal
        assert _attn(pv, page_size=256, v=_pool(256 if pv == "f8" else 64), max_pages=1, P=1, D=128) == -5


# every single-fault argument of the table, for all three entry points
_TABLE_FAULTS = [(dict(page_size=32), -1), (dict(page_size=16), -1), (dict(page_size=96), -1), (dict(page_size=512), -1),
                 (dict(page_size=0), -1), (dict(table=None), -1), (dict(table=FAKE + 2), -1), (dict(table=FAKE + 1), -1),
                 (dict(max_pages=0), -1), (dict(max_pages=-1), -1), (dict(P=0), -1), (dict(P=-3), -1), (dict(tstride=4), -1),
                 (dict(tstride=0), -1), (dict(max_pages=1 << 24, tstride=1 << 24, page_size=256), -4)]


@no_gpu
def test_append_status_table():
    """Each argument made invalid on its own returns its argument status: nothing was launched (a launch returns -5 here)."""
    from sageattention_amd import _lib as L
    odd = L.SageTensor(FAKE + 8, 1 << 16, 1 << 13, 64)
    cases = _TABLE_FAULTS + [
        (dict(k=None), -1), (dict(k8=None), -1), (dict(km=None), -1), (dict(ks=None), -1), (dict(start=None), -1),
        (dict(lens=None), -1), (dict(km=FAKE + 8), -1), (dict(coef=FAKE + 8), -1), (dict(start=FAKE + 2), -1),
        (dict(lens=FAKE + 1), -1), (dict(k=odd), -1), (dict(k8=odd), -1), (dict(v=odd), -1), (dict(v8=odd), -1),
        (dict(k=_pool(68)), -1), (dict(max_new=0), -1), (dict(max_new=-1), -1), (dict(coef=None), -1), (dict(v=None), -1),
        (dict(D=96), -2), (dict(D=32), -2), (dict(D=256), -2), (dict(gran=2), -1), (dict(gran=0), -1), (dict(gran=4), -1),
        (dict(rnd=2), -1), (dict(dt=2), -1), (dict(B=0), -1), (dict(H=0), -1)]
    wrong = [(sorted(c), st, got) for c, st in cases if (got := _append(**c)) != st]
    assert not wrong, wrong


@no_gpu
@pytest.mark.parametrize("pv", ["f16", "f8"])
def test_attention_status_table(pv):
    """... and for the two attention entry points: the table's faults, what is theirs, and what the contiguous split-KV entries
    answer for the arguments they share"""
    from sageattention_amd import _lib as L
    odd = L.SageTensor(FAKE + 8, 1 << 16, 1 << 12, 64)
    far = L.SageTensor(FAKE, 1 << 40, 1 << 36, 1 << 26)   # a (page, head) slice of 64 rows x 2^26 bytes: beyond the window
    cases = _TABLE_FAULTS + [
        (dict(lens=None), -1), (dict(lens=FAKE + 2), -1), (dict(k8=far), -4), (dict(v=far), -4),
        (dict(q=None), -1), (dict(k8=None), -1), (dict(v=None), -1), (dict(o=None), -1), (dict(ks=None), -1), (dict(km=None), -3),
        (dict(q=odd), -1), (dict(k8=odd), -1), (dict(v=odd), -1), (dict(km=FAKE + 8), -3), (dict(q_dt=2), -1), (dict(o_dt=2), -1),
        (dict(num_splits=0), -1), (dict(num_splits=17), -1), (dict(ws=None), -1), (dict(ws=FAKE + 8), -1), (dict(ws_bytes=16), -1),
        (dict(causal=1, q_fold=0), -1), (dict(causal=1, q_fold=3), -1), (dict(D=96), -2), (dict(D=32), -2), (dict(gran=1), -3),
        (dict(gran=0), -1), (dict(gran=4), -1), (dict(warpq=24), -1), (dict(sm_scale=0.0), -1), (dict(sm_scale=float("nan")), -1),
        (dict(B=0), -1), (dict(Hq=0), -1), (dict(Hk=0), -1), (dict(M=0), -1), (dict(Hq=3), -1)]
    cases += [(dict(v_scale=None), -1), (dict(v_scale=FAKE + 8), -1)] if pv == "f8" else [(dict(v_dt=2), -1)]
    wrong = [(sorted(c), st, got) for c, st in cases if (got := _attn(pv, **c)) != st]
    assert not wrong, wrong
    # a page slice that fits is addressed wherever the page lies: a page stride of 2^40 bytes is no fault
    assert _attn(pv, k8=L.SageTensor(FAKE, 1 << 40, 1 << 13, 64)) == -5


# ---- 3. Python refusals, raised before any device call ---------------------------------------------------------------------------
def _cpu_cache(pv="fp16", D=64, layout="HND", page_size=128, P=6, B=2):
    from sageattention_amd import SagePagedKVCache
    k = torch.zeros((P, 2, page_size, D) if layout == "HND" else (P, page_size, 2, D), dtype=torch.float16)
    c = SagePagedKVCache(k, k.clone(), pv, "per_thread", layout, 2.0)
    c.k8 = torch.zeros(k.shape, dtype=torch.int8)
    c.k_scale, c.km = torch.zeros(P, 2, page_size // 64 * 4), torch.zeros(B, 2, D, dtype=torch.float16)
    return c


def test_prepare_refusals():
    import sageattention_amd as sa
    from sageattention_amd import paged
    assert {"SagePagedKVCache", "sageattn_splitkv_paged"} <= set(sa.__all__) and sa.SagePagedKVCache is paged.SagePagedKVCache
    assert sa.sageattn_splitkv_paged is paged.sageattn_splitkv_paged
    k = torch.zeros(6, 2, 128, 64, dtype=torch.float16)
    table = torch.zeros(2, 3, dtype=torch.int32)
    lens = torch.tensor([80, 3], dtype=torch.int32)
    P = sa.SagePagedKVCache.prepare
    for bad in (32, 16, 96, 320, 512):
        kb = torch.zeros(6, 2, bad, 64, dtype=torch.float16)
        with pytest.raises(ValueError, match="page_size must be 64, 128 or 256.*64-key tiles"):
            P(kb, kb, table, lens)
    kb = torch.zeros(6, 32, 2, 64, dtype=torch.float16)      # NHD: the page size is the second dim
    with pytest.raises(ValueError, match="page_size"):
        P(kb, kb, table, lens, tensor_layout="NHD")
    with pytest.raises(ValueError, match="pv"):
        P(k, k, table, lens, pv="int8")
    with pytest.raises(ValueError, match="qk_quant_gran"):
        P(k, k, table, lens, qk_quant_gran="per_block")
    with pytest.raises(ValueError, match="layout"):
        P(k, k, table, lens, tensor_layout="BHSD")
    for bad in (72, 32, 256):
        kb = torch.zeros(6, 2, 128, bad, dtype=torch.float16)
        with pytest.raises(ValueError, match="head_dim 64 or 128"):
            P(kb, kb, table, lens)
    with pytest.raises(ValueError, match="one shape"):
        P(k, k[:, :1], table, lens)
    with pytest.raises(ValueError, match="one shape"):
        P(k, k[:5], table, lens)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        P(k.float(), k.float(), table, lens)
    with pytest.raises(ValueError, match="one dtype"):
        P(k, k.bfloat16(), table, lens)
    with pytest.raises(ValueError, match="16-byte aligned"):
        P(torch.zeros(6, 2, 128, 68, dtype=torch.float16)[..., 4:], k, table, lens)
    with pytest.raises(TypeError, match="v_headroom"):
        P(k, k, table, lens, v_headroom="2")
    for bad in (0.5, 0, float("nan")):
        with pytest.raises(ValueError, match="v_headroom"):
            P(k, k, table, lens, v_headroom=bad)
    _table_refusals(lambda t: P(k, k, t, lens), k.device)
    with pytest.raises(TypeError, match="int32"):
        P(k, k, table, lens.long())
    with pytest.raises(ValueError, match="kv_lens shape"):
        P(k, k, table, torch.zeros(3, dtype=torch.int32))


def _table_refusals(call, device, B=2):
    with pytest.raises(TypeError, match="block_table"):
        call([[0, 1, 2]] * B)
    with pytest.raises(TypeError, match="block_table must be of dtype int32"):
        call(torch.zeros(B, 3, dtype=torch.int64))
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(B, 3, 1, dtype=torch.int32), torch.zeros(B, 0, dtype=torch.int32)):
        with pytest.raises(ValueError, match="block_table shape"):
            call(bad)
    with pytest.raises(ValueError, match="block_table is on"):
        call(torch.zeros(B, 3, dtype=torch.int32, device="meta"))
    with pytest.raises(ValueError, match=r"stride\(-1\) == 1"):
        call(torch.zeros(B, 6, dtype=torch.int32)[:, ::2])
    with pytest.raises(ValueError, match=r"stride\(-1\) == 1"):
        call(torch.zeros(3, B, dtype=torch.int32).t())


def test_append_refusals():
    cache = _cpu_cache()
    table = torch.zeros(2, 3, dtype=torch.int32)
    lens = torch.tensor([80, 3], dtype=torch.int32)
    for bad in (1.0, "1", None, True, torch.tensor(1)):
        with pytest.raises(TypeError, match="max_new"):
            cache.append(table, lens, lens, bad)
    for bad in (0, -4):
        with pytest.raises(ValueError, match="max_new"):
            cache.append(table, lens, lens, bad)
    _table_refusals(lambda t: cache.append(t, lens, lens, 1), cache.k.device)
    with pytest.raises(ValueError, match="block_table shape"):
        cache.append(torch.zeros(3, 3, dtype=torch.int32), lens, lens, 1)     # three rows for a cache of two sequences
    with pytest.raises(TypeError, match="int32"):
        cache.append(table, lens.long(), lens, 1)
    with pytest.raises(TypeError, match="kv_lens"):
        cache.append(table, lens, [80, 3], 1)
    with pytest.raises(ValueError, match="kv_lens shape"):
        cache.append(table, lens, torch.zeros(3, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="is on"):
        cache.append(table, lens.to("meta"), lens, 1)


def test_attention_refusals():
    """what sageattn_splitkv_cached refuses is refused in the same words"""
    import sageattention_amd as sa
    cache = _cpu_cache()
    contiguous = sa.SageKVCache(torch.zeros(2, 2, 384, 64, dtype=torch.float16), torch.zeros(2, 2, 384, 64, dtype=torch.float16),
                                "fp16", "per_thread", "HND", 2.0)
    q = torch.zeros(2, 4, 8, 64, dtype=torch.float16)
    table = torch.zeros(2, 3, dtype=torch.int32)
    lens = torch.tensor([80, 3], dtype=torch.int32)
    f = sa.sageattn_splitkv_paged
    for causal in (False, True):
        for kw in (dict(is_causal=not causal), dict(attn_mask=torch.ones(8, 320, dtype=torch.bool)), dict(smooth_k=False),
                   dict(smooth_v=True), dict(block_map=torch.ones(1, 1, 1, 5, dtype=torch.bool)), dict(plan=object()),
                   dict(cu_seqlens_q=torch.zeros(3, dtype=torch.int32)), dict(cu_seqlens_k=torch.zeros(3, dtype=torch.int32))):
            with pytest.raises(ValueError, match="does not take") as e:
                f(q, cache, table, lens, 2, causal=causal, **kw)
            with pytest.raises(ValueError) as e2:
                sa.sageattn_splitkv_cached(q, contiguous, lens, 2, causal=causal, **kw)
            assert str(e.value) == str(e2.value)
        with pytest.raises(TypeError, match="unexpected keyword"):
            f(q, cache, table, lens, 2, causal=causal, window=3)
    with pytest.raises(TypeError, match="SagePagedKVCache"):
        f(q, contiguous, table, lens)
    with pytest.raises(TypeError, match="causal"):
        f(q, cache, table, lens, causal="yes")
    _table_refusals(lambda t: f(q, cache, t, lens), cache.k.device)
    with pytest.raises(TypeError, match="kv_lens"):
        f(q, cache, table, None)
    with pytest.raises(TypeError, match="int32"):
        f(q, cache, table, lens.long())
    with pytest.raises(ValueError, match="kv_lens shape"):
        f(q, cache, table, torch.zeros(3, dtype=torch.int32))
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="num_splits"):
            f(q, cache, table, lens, bad)
    with pytest.raises(TypeError, match="num_splits"):
        f(q, cache, table, lens, 2.0)
    with pytest.raises(TypeError, match="q_fold"):
        f(q, cache, table, lens, causal=True, q_fold=2.0)
    for bad in (0, 3, -1):
        with pytest.raises(ValueError, match="q_fold"):
            f(q, cache, table, lens, causal=True, q_fold=bad)
    with pytest.raises(ValueError, match="q_fold"):
        f(q, cache, table, lens, causal=False, q_fold=2)
    with pytest.raises(ValueError, match="head_dim"):
        f(torch.zeros(2, 4, 8, 128, dtype=torch.float16), cache, table, lens)
    with pytest.raises(ValueError, match="dtype"):
        f(q.bfloat16(), cache, table, lens)
    with pytest.raises(ValueError, match="divisible"):
        f(torch.zeros(2, 3, 8, 64, dtype=torch.float16), cache, table, lens, 2)


# ---- 4. the torch.library ops ------------------------------------------------------------------------------------------------------
def test_ops_live_in_their_own_namespace():
    import sageattention_amd  # noqa: F401
    import sageattention_amd.ops  # noqa: F401
    names = torch._C._dispatch_get_all_op_names()
    assert sorted(n.split("::")[1] for n in names if n.startswith(NS + "::")) == sorted(OPS)
    assert len([n for n in names if n.startswith("sageattention_amd::")]) == 26
    assert len([n for n in names if n.startswith("sageattention_amd_kvcache::")]) == 5
    ns = getattr(torch.ops, NS)
    s = str(ns.kv_cache_append_paged.default._schema)
    assert s.endswith("-> ()") and re.search(r"Tensor\(\w+!\) k8", s) and re.search(r"Tensor\(\w+!\) k_scale", s)
    assert re.search(r"Tensor\(\w+!\)\? v8", s) and "SymInt max_new" in s and "Tensor block_table" in s
    assert not re.search(r"Tensor\(\w+!\)\??\s+(k|v|km|v_coef|block_table|start_lens|kv_lens)\b", s)
    common = ("Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor block_table, Tensor kv_lens, "
              "SymInt num_splits, ")
    tail = "str tensor_layout, float sm_scale, str qk_quant_gran"
    for name in OPS[1:]:
        s = str(getattr(ns, name).default._schema)
        assert (common + ("SymInt q_fold, " if "causal" in name else "") + tail) in s, s
        assert "!" not in s                                              # nothing is mutated, block_table least of all
        assert s.endswith("-> (Tensor, Tensor)" if name.endswith("_lse") else "-> Tensor")


def _fake_state(cache, B):
    k, layout, fp8 = cache.k, cache.tensor_layout, cache.pv == "fp8"
    P, H, ps, D = (k.shape if layout == "HND" else (k.shape[0], k.shape[2], k.shape[1], k.shape[3]))
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=k.device)  # noqa: E731
    cache.k8 = z(k.shape, torch.int8)
    cache.k_scale, cache.km = z((P, H, ps // 64 * KU.gpb(cache)), torch.float32), z((B, H, D), k.dtype)
    if fp8:
        cache.v8 = z((P, H, D, ps) if layout == "HND" else (P, D, H, ps), torch.uint8).view(torch.float8_e4m3fn)
        cache.v_scale, cache.v_coef = z((B, H, D), torch.float32), z((B, H, 2, D), torch.float32)
    return cache


@pytest.mark.parametrize("layout", ["HND", "NHD"])
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_fakes_describe_their_outputs(layout, pv):
    """shape, dtype and stride of what the ops return: o contiguous in q's shape and dtype -- for a strided q as well --,
    lse fp32 [B, Hq, M] contiguous; the append returns nothing"""
    import sageattention_amd as sa
    with FakeTensorMode():
        D, B, HQ, M, P, ps = 128, 2, 4, 8, 7, 128
        k = torch.empty((P, 2, ps, D) if layout == "HND" else (P, ps, 2, D), dtype=torch.bfloat16, device="cuda")
        cache = _fake_state(sa.SagePagedKVCache(k, torch.empty_like(k), pv, "per_warp", layout, 2.0), B)
        lens = torch.empty((B,), dtype=torch.int32, device="cuda")
        table = torch.empty((B, 3), dtype=torch.int32, device="cuda")
        assert cache.append(table, lens, lens, 5) is None
        qshape = (B, HQ, M, D) if layout == "HND" else (B, M, HQ, D)
        big = torch.empty(tuple(2 * s for s in qshape), dtype=torch.bfloat16, device="cuda")
        for q in (torch.empty(qshape, dtype=torch.bfloat16, device="cuda"), big[:B, ::2, :qshape[2], D:]):
            contiguous = torch.empty(qshape).stride()
            for causal in (False, True):
                kw = dict(causal=causal, q_fold=4 if causal else 1)
                o = sa.sageattn_splitkv_paged(q, cache, table, lens, **kw)
                assert isinstance(o, torch.Tensor) and o.shape == q.shape and o.dtype == q.dtype and o.stride() == contiguous
                assert o.device == q.device
                o, lse = sa.sageattn_splitkv_paged(q, cache, table, lens, 3, return_lse=True, **kw)
                assert o.shape == q.shape and o.dtype == q.dtype and o.stride() == contiguous
                assert lse.shape == (B, HQ, M) and lse.dtype == torch.float32 and lse.is_contiguous() and lse.device == q.device
        c1 = cache.narrow(1, 1)
        assert c1.km.shape[0] == 1 and c1.k8 is cache.k8 and c1.k_scale is cache.k_scale and c1.k is cache.k
        assert (c1.v8 is None) == (pv == "fp16") and (pv == "fp16" or (c1.v8 is cache.v8 and c1.v_scale.shape[0] == c1.v_coef.shape[0] == 1))


# ---- 5. the tile-to-page arithmetic --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_size", PU.PAGE_SIZES)
def test_tile_homes_against_a_walk_over_rows(page_size):
    """every (start, len) on a small capacity: the tiles an append touches, mapped to (page, tile in page), against a walk over
    the ROWS of the rule -- row r of a sequence is row r % page_size of page table[r // page_size]"""
    N = 512
    max_pages = N // page_size
    row = [7 * i % 23 + 100 for i in range(max_pages)]        # distinct ids, not monotone
    assert len(set(row)) == max_pages
    for s in range(-1, N + 2):
        for n in list(range(-1, 200)) + [255, 256, 257, 448, 449, 511, 512, 513]:
            lc, sc = KU.clamp_len(n, N), KU.clamp_len(s, N)
            want_k, want_v = [], {64: [], 128: []}
            if lc > 0:
                first = min(sc, lc - 1) // 64 * 64               # the first row of the tile that holds row min(start, len - 1)
                for r in range(first, lc, 64):
                    want_k.append((row[r // page_size], (r % page_size) // 64))
                want_v[128] = list(want_k)
                first = first // 128 * 128                       # head_dim 64: a V workgroup holds the two blocks of a unit
                for r in range(first, lc, 64):
                    want_v[64].append((row[r // page_size], (r % page_size) // 64))
            assert PU.touched_k_homes(row, s, n, N, page_size) == want_k, (s, n)
            for D in (64, 128):
                assert PU.touched_v_homes(row, s, n, N, D, page_size) == want_v[D], (s, n, D)
            used = {p for p, _ in want_k} | {p for p, _ in want_v[64]}
            assert used <= set(row[:PU.pages_needed(lc, page_size)])   # no entry at or beyond ceil(len / page_size) is followed


def test_head_dim_64_unit_straddles_two_64_key_pages():
    row = [9, 4, 11, 2]
    # tiles 0 and 1 of a head_dim-64 unit are two PAGES at page_size 64, one page at 128
    assert PU.touched_v_homes(row, 64, 65, 256, 64, 64) == [(9, 0), (4, 0)]
    assert PU.touched_v_homes(row, 64, 65, 256, 64, 128) == [(9, 0), (9, 1)]
    assert PU.touched_v_homes(row, 64, 65, 256, 128, 64) == [(4, 0)]
    assert PU.touched_k_homes(row, 64, 65, 256, 64) == [(4, 0)]
    assert PU.touched_v_homes(row, 200, 130, 256, 64, 64) == [(11, 0)]       # rollback: the tile of row 129 alone (unit 1: blocks 2, 3)
    assert PU.tile_slot(5, 64) == (5, 0) and PU.tile_slot(5, 128) == (2, 1) and PU.tile_slot(5, 256) == (1, 1)
    with pytest.raises(AssertionError):
        PU.tiles_per_page(32)


def test_gather_follows_the_table():
    pool = torch.arange(5 * 2 * 64 * 4, dtype=torch.float32).reshape(5, 2, 64, 4)
    table = torch.tensor([[3, 0], [4, 4]], dtype=torch.int32)
    g = PU.gather(pool, table, "HND")
    assert g.shape == (2, 2, 128, 4)
    assert torch.equal(g[0, :, :64], pool[3]) and torch.equal(g[0, :, 64:], pool[0]) and torch.equal(g[1, :, 64:], pool[4])
    gn = PU.gather(pool.transpose(1, 2).contiguous(), table, "NHD")
    assert gn.shape == (2, 128, 2, 4) and torch.equal(gn.transpose(1, 2), g)
