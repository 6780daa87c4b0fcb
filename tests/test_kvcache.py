"""The persistent KV cache (``SageKVCache``, ``sageattn_splitkv_cached``, ``sage_kv_cache_append``) without a GPU: the tile
range of the rule, the new header against its ctypes table, the C status table, the Python refusals and the torch.library ops.
What the kernel computes: test_kvcache_gpu.py."""
import ctypes
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import kvcache_util as KU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = "sageattention_amd_kvcache"
OPS = ("kv_cache_append", "attn_splitkv_cached", "attn_splitkv_cached_lse", "attn_splitkv_causal_cached",
       "attn_splitkv_causal_cached_lse")


# ---- 1. the tile range of the rule ---------------------------------------------------------------------------------------------
def test_touched_tiles_edges():
    T = lambda s, l, N=320: list(KU.touched_tiles(s, l, N))  # noqa: E731
    assert T(0, 0) == [] and T(200, 0) == [] and T(0, -3) == []           # no keys: nothing, whatever start says
    assert T(0, 1) == [0]
    assert T(130, 130) == [2] and T(128, 128) == [1] and T(129, 129) == [2]   # start = len: the tile of row len - 1
    assert T(200, 130) == [2] and T(320, 1) == [0]                          # start > len (rollback): the same tile
    assert T(63, 64) == [0] and T(64, 65) == [1] and T(62, 63) == [0]      # len at, above and below a tile edge
    assert T(0, 64) == [0] and T(0, 65) == [0, 1] and T(0, 63) == [0]
    assert T(100, 130) == [1, 2] and T(60, 200) == [0, 1, 2, 3] and T(319, 320) == [4]
    assert T(-5, 400) == [0, 1, 2, 3, 4] and T(-5, 1) == [0] and T(1000, 1000) == [4]   # clamped to [0, N]
    assert T(0, 100, 70) == [0, 1] and T(69, 70, 70) == [1]
    for N in (1, 64, 70, 320):
        for s in range(-2, N + 3, 7):
            for l in range(-2, N + 3, 5):
                t = KU.touched_tiles(s, l, N)
                lc, sc = KU.clamp_len(l, N), KU.clamp_len(s, N)
                if lc == 0:
                    assert len(t) == 0
                    continue
                assert t.stop == (lc + 63) // 64 and t.start <= (lc - 1) // 64 and t.start * 64 <= min(sc, lc - 1) < t.start * 64 + 64
                assert len(t) <= (KU.need(s, l, N) + 63) // 64 + 1          # the K slots of the grid cover it


def test_touched_v_blocks():
    assert list(KU.touched_v_blocks(64, 65, 320, 128)) == [1]
    assert list(KU.touched_v_blocks(64, 65, 320, 64)) == [0, 1]           # a head_dim-64 unit holds blocks 0 and 1
    assert list(KU.touched_v_blocks(130, 130, 320, 64)) == [2] and list(KU.touched_v_blocks(0, 0, 320, 64)) == []


# ---- 2. the new header against its table -----------------------------------------------------------------------------------------
def _prototypes(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    ctype = lambda s: re.sub(r"\bconst\b|\s", "", s)  # noqa: E731
    out = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\s*\b(sage_\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = (ctype(ret), [ctype(re.sub(r"\w+$", "", p.strip())) for p in params.split(",")])
    return out


def test_kvcache_header_matches_its_table():
    from sageattention_amd import _lib as L
    protos = _prototypes("sageattn_hip_kvcache.h")
    assert sorted(protos) == sorted(L.KVCACHE_SIGNATURES) == ["sage_kv_cache_append"]
    want = {"int": ctypes.c_int, "sage_stream_t": ctypes.c_void_p}
    for name, (ret, params) in protos.items():
        res, args = L.KVCACHE_SIGNATURES[name]
        assert res is want[ret] and len(params) == len(args) == 18
        for c, ct in zip(params, args):
            if c == "sage_tensor*":
                assert ct is ctypes.POINTER(L.SageTensor), (name, c)
            elif c.endswith("*"):
                assert c[:-1] in ("void", "float", "int32_t") and ct is ctypes.c_void_p, (name, c)
            else:
                assert ct is want[c], (name, c)
    # the main header and its table are what they were
    assert len(sorted(L.SIGNATURES)) == 69 and not set(L.SIGNATURES) & set(L.KVCACHE_SIGNATURES)
    assert "sage_kv_cache_append" not in open(os.path.join(ROOT, "include", "sageattn_hip.h")).read()
    assert L.lib().sage_abi_version() == 3


def test_symbol_exported_and_bound():
    from sageattention_amd import _lib as L
    fn = L.lib().sage_kv_cache_append
    assert fn.restype is ctypes.c_int and fn.argtypes == L.KVCACHE_SIGNATURES["sage_kv_cache_append"][1]


# ---- 3. the C status table -------------------------------------------------------------------------------------------------------
# Fake device addresses: where a GPU is visible a missed check would launch kernels on them, so this runs only where none
# is; there every launch attempt returns SAGE_ERR_LAUNCH (-5), which makes a launch observable (tests/test_cabi_symbols.py).
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")
FAKE = 1 << 20
_PARAMS = "k v dt B H N D km k8 ks gran rnd v8 coef start lens max_new stream"


def _call(**change):
    from sageattention_amd import _lib as L
    t = L.SageTensor(FAKE, 1 << 16, 1 << 12, 64)
    vt = L.SageTensor(FAKE, 1 << 16, 1 << 12, 320)
    args = dict(k=t, v=t, dt=0, B=2, H=2, N=320, D=64, km=FAKE, k8=t, ks=FAKE, gran=3, rnd=0, v8=vt, coef=FAKE, start=FAKE,
                lens=FAKE, max_new=1, stream=None)
    args.update(change)
    return L.lib().sage_kv_cache_append(*[args[n] for n in _PARAMS.split()])


@no_gpu
def test_valid_calls_reach_a_launch():
    from sageattention_amd import _lib as L
    assert _call() == -5
    assert _call(v=None, v8=None, coef=None) == -5                      # FP16 / BF16 P.V: no V half
    assert _call(v8=None) == -5 and _call(v8=None, coef=None) == -5       # v and v_coef are not read without v_fp8
    assert _call(gran=1, rnd=1, dt=1, D=128, max_new=1 << 30) == -5
    assert _call(start=FAKE + 4, lens=FAKE + 8, km=FAKE + 16, coef=FAKE + 32) == -5
    assert _call(k=L.SageTensor(FAKE, 1 << 16, 64, 128), N=1) == -5


@no_gpu
def test_status_table():
    """Each argument made invalid on its own returns its argument status: nothing was launched (a launch returns -5 here)."""
    from sageattention_amd import _lib as L
    odd = L.SageTensor(FAKE + 8, 1 << 16, 1 << 12, 64)
    odd_stride = L.SageTensor(FAKE, 1 << 16, 1 << 12, 68)
    cases = [(dict(k=None), -1), (dict(k8=None), -1), (dict(km=None), -1), (dict(ks=None), -1), (dict(start=None), -1),
             (dict(lens=None), -1), (dict(km=FAKE + 8), -1), (dict(coef=FAKE + 8), -1), (dict(start=FAKE + 2), -1),
             (dict(lens=FAKE + 1), -1), (dict(k=odd), -1), (dict(k8=odd), -1), (dict(v=odd), -1), (dict(v8=odd), -1),
             (dict(k=odd_stride), -1), (dict(max_new=0), -1), (dict(max_new=-1), -1), (dict(coef=None), -1), (dict(v=None), -1),
             (dict(D=96), -2), (dict(D=32), -2), (dict(D=256), -2),
             (dict(gran=2), _k_smooth_quant_status(gran=2)), (dict(gran=0), -1), (dict(gran=4), -1), (dict(rnd=2), -1),
             (dict(dt=2), -1), (dict(B=0), -1), (dict(H=0), -1), (dict(N=0), -1)]
    wrong = [(sorted(c), st, got) for c, st in cases if (got := _call(**c)) != st]
    assert not wrong, wrong
    assert _k_smooth_quant_status(gran=2) == -1


def _k_smooth_quant_status(gran):
    """what sage_k_smooth_quant answers for this K granularity"""
    from sageattention_amd import _lib as L
    t = L.SageTensor(FAKE, 1 << 16, 1 << 12, 64)
    return L.lib().sage_k_smooth_quant(t, 0, 2, 2, 320, 64, t, FAKE, FAKE, gran, 0, FAKE, None)


# ---- 4. Python refusals, raised before any device call ---------------------------------------------------------------------------
def _cpu_cache(pv="fp16", D=64, layout="HND"):
    from sageattention_amd import SageKVCache
    k = torch.zeros((2, 2, 320, D) if layout == "HND" else (2, 320, 2, D), dtype=torch.float16)
    return SageKVCache(k, k.clone(), pv, "per_thread", layout, 2.0)


def test_prepare_refusals():
    import sageattention_amd as sa
    from sageattention_amd import kvcache
    assert {"SageKVCache", "sageattn_splitkv_cached"} <= set(sa.__all__) and sa.SageKVCache is kvcache.SageKVCache
    assert sa.sageattn_splitkv_cached is kvcache.sageattn_splitkv_cached
    k = torch.zeros(2, 2, 320, 64, dtype=torch.float16)
    lens = torch.tensor([80, 3], dtype=torch.int32)
    P = sa.SageKVCache.prepare
    with pytest.raises(ValueError, match="pv"):
        P(k, k, lens, pv="int8")
    with pytest.raises(ValueError, match="qk_quant_gran"):
        P(k, k, lens, qk_quant_gran="per_block")
    with pytest.raises(ValueError, match="layout"):
        P(k, k, lens, tensor_layout="BHSD")
    for bad in (72, 32, 256):
        with pytest.raises(ValueError, match="head_dim 64 or 128"):
            P(torch.zeros(2, 2, 320, bad, dtype=torch.float16), torch.zeros(2, 2, 320, bad, dtype=torch.float16), lens)
    with pytest.raises(ValueError, match="one shape"):
        P(k, k[:, :1], lens, pv="fp8")
    with pytest.raises(ValueError, match="fp16 or bf16"):
        P(k.float(), k.float(), lens)
    with pytest.raises(ValueError, match="16-byte aligned"):
        P(torch.zeros(2, 2, 320, 68, dtype=torch.float16)[..., 4:], k, lens)
    with pytest.raises(TypeError, match="v_headroom"):
        P(k, k, lens, v_headroom="2")
    for bad in (0.5, 0, float("nan")):
        with pytest.raises(ValueError, match="v_headroom"):
            P(k, k, lens, v_headroom=bad)
    with pytest.raises(TypeError, match="int32"):
        P(k, k, lens.long())
    with pytest.raises(ValueError, match="kv_lens shape"):
        P(k, k, torch.zeros(3, dtype=torch.int32))


def test_append_refusals():
    cache = _cpu_cache()
    lens = torch.tensor([80, 3], dtype=torch.int32)
    for bad in (1.0, "1", None, True, torch.tensor(1)):
        with pytest.raises(TypeError, match="max_new"):
            cache.append(lens, lens, bad)
    for bad in (0, -4):
        with pytest.raises(ValueError, match="max_new"):
            cache.append(lens, lens, bad)
    with pytest.raises(TypeError, match="int32"):
        cache.append(lens.long(), lens, 1)
    with pytest.raises(TypeError, match="kv_lens"):
        cache.append(lens, [80, 3], 1)
    with pytest.raises(ValueError, match="kv_lens shape"):
        cache.append(lens, torch.zeros(3, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="is on"):
        cache.append(lens.to("meta"), lens, 1)


def test_attention_refusals():
    """what sageattn_splitkv / sageattn_splitkv_causal refuse by name is refused in the same words"""
    import sageattention_amd as sa
    cache = _cpu_cache()
    q = torch.zeros(2, 4, 8, 64, dtype=torch.float16)
    lens = torch.tensor([80, 3], dtype=torch.int32)
    f = sa.sageattn_splitkv_cached
    for causal, op in ((False, "sageattn_splitkv"), (True, "sageattn_splitkv_causal")):
        for kw in (dict(is_causal=not causal), dict(attn_mask=torch.ones(8, 320, dtype=torch.bool)), dict(smooth_k=False),
                   dict(smooth_v=True), dict(block_map=torch.ones(1, 1, 1, 5, dtype=torch.bool)), dict(plan=object()),
                   dict(cu_seqlens_q=torch.zeros(3, dtype=torch.int32)), dict(cu_seqlens_k=torch.zeros(3, dtype=torch.int32))):
            with pytest.raises(ValueError, match=f"{op} does not take") as e:
                f(q, cache, lens, 2, causal=causal, **kw)
            with pytest.raises(ValueError) as e2:
                getattr(sa, op)(q, cache.k, cache.v, lens, 2, **kw)
            assert str(e.value) == str(e2.value)
        with pytest.raises(TypeError, match="unexpected keyword"):
            f(q, cache, lens, 2, causal=causal, window=3)
    with pytest.raises(TypeError, match="SageKVCache"):
        f(q, (cache.k, cache.v), lens)
    with pytest.raises(TypeError, match="causal"):
        f(q, cache, lens, causal="yes")
    with pytest.raises(TypeError, match="int32"):
        f(q, cache, lens.long())
    with pytest.raises(ValueError, match="kv_lens shape"):
        f(q, cache, torch.zeros(3, dtype=torch.int32))
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="num_splits"):
            f(q, cache, lens, bad)
    with pytest.raises(TypeError, match="num_splits"):
        f(q, cache, lens, 2.0)
    with pytest.raises(TypeError, match="q_fold"):
        f(q, cache, lens, causal=True, q_fold=2.0)
    for bad in (0, 3, -1):
        with pytest.raises(ValueError, match="q_fold"):
            f(q, cache, lens, causal=True, q_fold=bad)
    with pytest.raises(ValueError, match="q_fold"):
        f(q, cache, lens, causal=False, q_fold=2)
    with pytest.raises(ValueError, match="head_dim"):
        f(torch.zeros(2, 4, 8, 128, dtype=torch.float16), cache, lens)
    with pytest.raises(ValueError, match="dtype"):
        f(q.bfloat16(), cache, lens)
    with pytest.raises(ValueError, match="divisible"):
        f(torch.zeros(2, 3, 8, 64, dtype=torch.float16), _fake_state(cache), lens, 2)


# ---- 5. the torch.library ops ------------------------------------------------------------------------------------------------------
def test_ops_live_in_their_own_namespace():
    import sageattention_amd  # noqa: F401
    import sageattention_amd.ops  # noqa: F401
    names = torch._C._dispatch_get_all_op_names()
    assert sorted(n.split("::")[1] for n in names if n.startswith(NS + "::")) == sorted(OPS)
    assert len([n for n in names if n.startswith("sageattention_amd::")]) == 26
    ns = getattr(torch.ops, NS)
    s = str(ns.kv_cache_append.default._schema)
    assert s.endswith("-> ()") and re.search(r"Tensor\(\w+!\) k8", s) and re.search(r"Tensor\(\w+!\) k_scale", s)
    assert re.search(r"Tensor\(\w+!\)\? v8", s) and "SymInt max_new" in s
    assert not re.search(r"Tensor\(\w+!\)\??\s+(k|v|km|v_coef|start_lens|kv_lens)\b", s)
    common = "Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor? kv_lens, SymInt num_splits, "
    tail = "str tensor_layout, float sm_scale, str qk_quant_gran"
    for name in OPS[1:]:
        s = str(getattr(ns, name).default._schema)
        assert (common + ("SymInt q_fold, " if "causal" in name else "") + tail) in s, s
        assert s.endswith("-> (Tensor, Tensor)" if name.endswith("_lse") else "-> Tensor")


def _fake_state(cache, dev=None):
    """state tensors of the shapes ``prepare`` gives, without a device call (zeros on k's device)"""
    k, layout, fp8 = cache.k, cache.tensor_layout, cache.pv == "fp8"
    B, H, N, D = (k.shape if layout == "HND" else (k.shape[0], k.shape[2], k.shape[1], k.shape[3]))
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=k.device)  # noqa: E731
    cache.k8 = z((B, H, N, D), torch.int8) if layout == "HND" else z((B, H, N, D), torch.int8).transpose(1, 2)
    cache.k_scale, cache.km = z((B, H, (N + 63) // 64 * 4), torch.float32), z((B, H, D), k.dtype)
    if fp8:
        npad = (N + 63) // 64 * 64
        cache.v8 = z((B, H, D, npad) if layout == "HND" else (B, D, H, npad), torch.uint8).view(torch.float8_e4m3fn)
        cache.v_scale, cache.v_coef = z((B, H, D), torch.float32), z((B, H, 2, D), torch.float32)
    return cache


@pytest.mark.parametrize("layout", ["HND", "NHD"])
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_fakes_describe_their_outputs(layout, pv):
    """shape, dtype and stride of what the ops return: o contiguous in q's shape and dtype -- for a strided q as well --,
    lse fp32 [B, Hq, M] contiguous; the append returns nothing"""
    import sageattention_amd as sa
    with FakeTensorMode():
        from sageattention_amd import SageKVCache
        D, B, HQ, M = 128, 2, 4, 8
        k = torch.empty((B, 2, 320, D) if layout == "HND" else (B, 320, 2, D), dtype=torch.bfloat16, device="cuda")
        cache = _fake_state(SageKVCache(k, torch.empty_like(k), pv, "per_warp", layout, 2.0))
        lens = torch.empty((B,), dtype=torch.int32, device="cuda")
        assert cache.append(lens, lens, 5) is None
        qshape = (B, HQ, M, D) if layout == "HND" else (B, M, HQ, D)
        big = torch.empty(tuple(2 * s for s in qshape), dtype=torch.bfloat16, device="cuda")
        for q in (torch.empty(qshape, dtype=torch.bfloat16, device="cuda"), big[:B, ::2, :qshape[2], D:]):
            contiguous = torch.empty(qshape).stride()
            for causal in (False, True):
                kw = dict(causal=causal, q_fold=4 if causal else 1)
                o = sa.sageattn_splitkv_cached(q, cache, lens, **kw)
                assert isinstance(o, torch.Tensor) and o.shape == q.shape and o.dtype == q.dtype and o.stride() == contiguous
                assert o.device == q.device
                o, lse = sa.sageattn_splitkv_cached(q, cache, None, 3, return_lse=True, **kw)
                assert o.shape == q.shape and o.dtype == q.dtype and o.stride() == contiguous
                assert lse.shape == (B, HQ, M) and lse.dtype == torch.float32 and lse.is_contiguous() and lse.device == q.device
        c1 = cache.narrow(1, 1)
        assert c1.k.shape[0] == c1.k8.shape[0] == c1.k_scale.shape[0] == c1.km.shape[0] == 1
        assert (c1.v8 is None) == (pv == "fp16") and (pv == "fp16" or c1.v8.shape[0] == c1.v_scale.shape[0] == c1.v_coef.shape[0] == 1)
