"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/sageattn_hip.h declares.
No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    from sageattention_amd import _build
    return _build.build()


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "sageattn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sage_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported(built_lib):
    lib = ctypes.CDLL(built_lib)
    names = _declared_symbols()
    assert len(names) >= 13, names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/sageattn_hip.h but not exported"


def test_binding_covers_header(built_lib):
    from sageattention_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared_symbols()
    l = _lib.lib()
    assert l.sage_abi_version() == 3
    assert l.sage_target_arch() == b"gfx950"
    assert b"head_dim" in l.sage_status_string(-2)


def test_argument_validation_without_gpu(built_lib):
    """Host-side validation returns status codes before anything touches a device."""
    from sageattention_amd import _lib as L
    l = L.lib()
    t = L.SageTensor(None, 0, 0, 0)
    assert l.sage_k_mean(t, 0, 1, 1, 1, 64, None, None, None) == -1
    bad = L.SageTensor(16, 8, 8, 8)
    assert l.sage_quant_qk_int8(bad, 0, 1, 1, 8, 96, None, bad, 16, 1, 0, 128, 128, 1.0, 0, None, 1, None, None) == -2
    assert l.sage_quant_qk_int8(bad, 7, 1, 1, 8, 64, None, bad, 16, 1, 0, 128, 128, 1.0, 0, None, 1, None, None) == -1
    assert l.sage_set_tuning(0, 5) == -1 and l.sage_set_tuning(0, 0) == 0
    assert l.sage_set_tuning(1, 1) == -1
    assert l.sage_set_tuning(0, 8) == 0 and l.sage_get_tuning(0) == 8 and l.sage_set_tuning(0, 0) == 0
    assert l.sage_get_tuning(0) == 0 and l.sage_get_tuning(9) == -1
    assert l.sage_set_tuning(7, 0) == -1


def test_sequence_parallel_entry_points_validate_arguments(built_lib):
    """The round-2 building blocks (kv tile layouts, statistics, tile-major quantizers, merge_ex) reject bad arguments on
    the host, before any launch."""
    import ctypes as C
    from sageattention_amd import _lib as L
    l = L.lib()
    t = L.SageTensor(16, 64, 64, 64)
    lay = L.KvLayout(0, 0, 0, 0, 0)
    args = (1, 1, 1, 64, 64, 64, 0, 3, 128, 32, 0.125, None)
    assert l.sage_attn_qk_int8_pv_f16_kvtiles(t, t, t, 0, t, 0, 16, 16, None, None, *args) == -1          # no layout
    assert l.sage_attn_qk_int8_pv_f8_kvtiles(t, t, t, t, 0, 16, 16, 16, None, None, *args) == -1
    bad = L.KvLayout(-64, 0, 0, 0, 0)
    assert l.sage_attn_qk_int8_pv_f16_kvtiles(t, t, t, 0, t, 0, 16, 16, bad, None, *args) == -1           # negative stride
    odd = L.KvLayout(0, 0, 6, 2, 2)
    assert l.sage_attn_qk_int8_pv_f16_kvtiles(t, t, t, 0, t, 0, 16, 16, odd, None, *args) == -1           # scale strides < 4
    assert l.sage_seq_stats(t, 0, 1, 1, 64, 96, 16, 16, None) == -2                                       # head_dim
    assert l.sage_seq_stats(t, 0, 1, 1, 64, 64, None, 16, None) == -1
    assert l.sage_kv_stats_reduce(None, None, 1, 192, 1, 64, 64, 0, 448.0, None, None, None, None) == -1
    assert l.sage_kv_stats_reduce(16, None, 2, 10, 1, 64, 64, 0, 448.0, 16, None, None, None) == -1       # part stride too small
    st3 = (C.c_int64 * 3)(4, 4, 4)
    assert l.sage_quant_k_int8_kvtiles(t, 0, 1, 1, 64, 64, None, t, 0, 16, st3, 3, 0, None) == -1         # no tile stride
    assert l.sage_quant_k_int8_kvtiles(t, 0, 1, 1, 64, 64, None, t, 4096, 16, st3, 2, 0, None) == -1      # per_warp is a Q granularity
    assert l.sage_quant_v_fp8_apply(t, 0, 1, 1, 64, 64, t, 24, 16, None) == -1                            # unaligned tile stride
    assert l.sage_k_smooth_quant(t, 0, 1, 1, 64, 64, t, 16, None, 3, 0, 16, None) == -1                   # km missing
    assert l.sage_kv_prepare_fp8(t, t, 0, 1, 1, 64, 64, t, 16, None, 3, 0, t, 16, 448.0, 16, None) == -1  # km missing
    assert l.sage_kv_prepare_fp8(t, t, 0, 1, 1, 64, 96, t, 16, 16, 3, 0, t, 16, 448.0, 16, None) == -2    # head_dim
    assert l.sage_kv_prepare_fp8(t, t, 0, 1, 1, 64, 64, t, 16, 16, 2, 0, t, 16, 448.0, 16, None) == -1    # per_warp is a Q granularity
    assert l.sage_kv_prepare_fp8_workspace_bytes(2, 3, 1000, 64) >= 2 * 2 * 3 * 4 * 64 * 4
    op = (C.c_void_p * 1)(16)
    assert l.sage_merge_attn_states_multi_ex(op, op, 1, 0, 16, None, 4, 64, 0.0, None, 0.0, None) == -1   # lse multiplier must be > 0


def test_one_call_operator_validates_arguments(built_lib):
    """sage_sageattn_pv_{f16,f8}: workspace sizing and host-side validation, no launch."""
    from sageattention_amd import _lib as L
    l = L.lib()
    t = L.SageTensor(16, 64, 64, 64)
    ok = L.OpOpts(3, 32, 1, -1, 0)
    n16 = l.sage_sageattn_workspace_bytes(0, 2, 4, 2, 1000, 1000, 64, 1, ok)
    n8 = l.sage_sageattn_workspace_bytes(1, 2, 4, 2, 1000, 1000, 64, 1, ok)
    assert n16 >= 2 * 2 * 1000 * 64 and n8 >= n16 + 2 * 2 * 64 * 1024              # int8 K; + fp8 V^T
    big = l.sage_sageattn_workspace_bytes(0, 1, 4, 2, 8192, 8192, 128, 1, L.OpOpts(3, 32, 1, 0, 0))  # fuse_q = 0: stand-alone Q quantizer
    assert big >= 2 * 8192 * 128 + 4 * 8192 * 128 + 2 * 4 * 8192 * 4
    assert l.sage_sageattn_workspace_bytes(0, 1, 1, 1, 64, 64, 96, 0, ok) == 0       # head_dim
    assert l.sage_sageattn_workspace_bytes(0, 1, 1, 1, 64, 64, 64, 0, L.OpOpts(1, 32, 1, -1, 0)) == 0  # per_block: not here
    args = (1, 2, 2, 64, 64, 64, 0, 0.125)
    assert l.sage_sageattn_pv_f16(t, t, t, 0, t, None, *args, ok, 16, 8, None) == -1             # workspace too small
    assert l.sage_sageattn_pv_f16(t, t, t, 0, t, None, *args, ok, None, 1 << 20, None) == -1
    assert l.sage_sageattn_pv_f16(t, t, t, 0, t, None, *args, L.OpOpts(3, 32, 0, -1, 0), 16, 1 << 20, None) == -3  # smooth_k = 0
    assert l.sage_sageattn_pv_f16(t, t, t, 0, t, None, *args, L.OpOpts(3, 32, 1, -1, 5), 16, 1 << 20, None) == -1  # nwaves
    assert l.sage_sageattn_pv_f16(t, t, t, 0, t, None, 1, 3, 2, 64, 64, 64, 0, 0.125, ok, 16, 1 << 20, None) == -1  # Hq % Hk
    assert l.sage_sageattn_pv_f8(t, t, t, 0, t, None, *args, 0.0, ok, 16, 1 << 20, None) == -1   # scale_max


def test_product_path_has_no_oracle_import():
    """The shipped package must never import the oracle or fall back to CPU."""
    pkg = os.path.join(ROOT, "sageattention_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"^\s*(from|import)\s+[^#\n]*oracle", src, flags=re.M), fn
            assert "sage_oracle" not in src, fn


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from sageattention_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


# ---- every argument is checked before the first launch ------------------------------------------------------------------
# The cases below pass fake device addresses.  Where a GPU is visible a missed check would launch kernels on them, so they
# run only where none is: there every launch attempt returns SAGE_ERR_LAUNCH (-5), which makes a launch observable.
def _gpu_visible():
    import torch
    return torch.cuda.is_available()


no_gpu = pytest.mark.skipif(_gpu_visible(), reason="passes fake device addresses: only where no GPU is visible")

FAKE = 1 << 20  # a 16-byte aligned fake device address
ODD = FAKE + 8  # an unaligned one

# parameter names of every entry point that validates its arguments, in the order of include/sageattn_hip.h
_PARAMS = {
    "sage_k_mean": "k dtype B H N D km ws stream",
    "sage_quant_qk_int8": "x dtype B H N D mean out scale gran is_key blk warp mult rounding dvec dgroup dot stream",
    "sage_quant_qk_int8_varlen": "x dtype cu nseq H N D mean out scale gran is_key blk warp mult rounding stream",
    "sage_sub_mean_f16": "v dtype B H N D vm out stream",
    "sage_quant_k_int8_kvtiles": "k dtype B H N D mean out tile scale sstr gran rounding stream",
    "sage_k_smooth_quant": "k dtype B H N D out scale km gran rounding ws stream",
    "sage_kv_prepare_fp8": "k v dtype B H N D k8 ks km gran rounding v8 vs smax ws stream",
    "sage_quant_v_fp8": "v dtype B H N D v8 vs vm smax ws stream",
    "sage_seq_stats": "x dtype B H N D stats ws stream",
    "sage_kv_stats_reduce": "kst vst parts pstride BH D n dtype smax km vs vc stream",
    "sage_quant_v_fp8_apply": "v dtype B H N D v8 tile vc stream",
    "sage_merge_attn_states": "oa la ob dtype lb rows D stream",
    "sage_merge_attn_states_multi_ex": "obs lbs count dtype oo lo rows D mult corr cmult stream",
    "sage_merge_attn_states_multi": "obs lbs count dtype oo lo rows D stream",
    "sage_finish_lse": "l2 corr sm lo n stream",
    "sage_attn_qk_int8_pv_f16": "q k v vdt o odt qs ks vm lse B Hq Hk M N D causal gran blkq warpq sm lm1 stream",
    "sage_attn_qk_int8_pv_f8": "q k v o odt qs ks vs vm lse B Hq Hk M N D causal gran blkq warpq sm lm1 stream",
    "sage_attn_qk_int8_pv_f16_varlen": "q k v vdt o odt qs ks cuq cuk B Hq Hk M N D causal gran blkq warpq sm lm1 stream",
    "sage_attn_fusedq_pv_f16": "q qdt k v vdt o odt ks km vm lse B Hq Hk M N D causal gran warpq sm stream",
    "sage_attn_fusedq_pv_f8": "q qdt k v o odt ks km vs vm lse B Hq Hk M N D causal gran warpq sm stream",
    "sage_attn_qk_int8_pv_f16_masked": "q k v vdt o odt qs ks mask mkind mstr lse B Hq Hk M N D gran blkq warpq sm lm1 stream",
    "sage_attn_qk_int8_pv_f16_kvtiles": "q k v vdt o odt qs ks lay lse B Hq Hk M N D causal gran blkq warpq sm stream",
    "sage_attn_qk_int8_pv_f8_kvtiles": "q k v o odt qs ks vs lay lse B Hq Hk M N D causal gran blkq warpq sm stream",
    "sage_sageattn_pv_f16": "q k v dtype o lse B Hq Hk M N D causal sm opts ws wsb stream",
    "sage_sageattn_pv_f8": "q k v dtype o lse B Hq Hk M N D causal sm smax opts ws wsb stream",
}


def _t(data=FAKE, sn=64):
    from sageattention_amd import _lib as L
    return L.SageTensor(data, 1 << 16, 1 << 12, sn)


def _valid_args():
    """One valid argument set per entry point (every pointer a fake address)."""
    import ctypes as C
    from sageattention_amd import _lib as L
    t, a = _t(), FAKE
    shape = dict(dtype=0, B=1, H=1, N=64, D=64, stream=None)
    quant = dict(shape, x=t, mean=None, out=t, scale=a, gran=3, is_key=0, blk=128, warp=32, mult=1.0, rounding=0)
    attn = dict(q=t, k=t, v=t, vdt=0, o=t, odt=0, qs=a, ks=a, vs=a, vm=None, lse=None, B=1, Hq=2, Hk=1, M=64, N=64, D=64,
                causal=0, gran=3, blkq=128, warpq=32, sm=0.125, lm1=0, stream=None)
    blks = (C.c_void_p * 16)(*([a] * 16))
    op = dict(q=t, k=t, v=t, dtype=0, o=t, lse=None, B=1, Hq=2, Hk=1, M=64, N=64, D=64, causal=0, sm=0.125, smax=448.0,
              opts=L.OpOpts(3, 32, 1, -1, 0), ws=a, wsb=1 << 40, stream=None)
    return {
        "sage_k_mean": dict(shape, k=t, km=a, ws=a),
        "sage_quant_qk_int8": dict(quant, dvec=None, dgroup=1, dot=None),
        "sage_quant_qk_int8_varlen": dict(quant, cu=a, nseq=1),
        "sage_sub_mean_f16": dict(shape, v=t, vm=a, out=t),
        "sage_quant_k_int8_kvtiles": dict(shape, k=t, mean=None, out=t, tile=4096, scale=a, sstr=(C.c_int64 * 3)(256, 256, 4),
                                          gran=3, rounding=0),
        "sage_k_smooth_quant": dict(shape, k=t, out=t, scale=a, km=a, gran=3, rounding=0, ws=a),
        "sage_kv_prepare_fp8": dict(shape, k=t, v=t, k8=t, ks=a, km=a, gran=3, rounding=0, v8=t, vs=a, smax=448.0, ws=a),
        "sage_quant_v_fp8": dict(shape, v=t, v8=t, vs=a, vm=None, smax=448.0, ws=a),
        "sage_seq_stats": dict(shape, x=t, stats=a, ws=a),
        "sage_kv_stats_reduce": dict(kst=a, vst=a, parts=1, pstride=384, BH=1, D=64, n=64, dtype=0, smax=448.0, km=a, vs=a,
                                     vc=a, stream=None),
        "sage_quant_v_fp8_apply": dict(shape, v=t, v8=t, tile=0, vc=a),
        "sage_merge_attn_states": dict(oa=a, la=a, ob=a, dtype=0, lb=a, rows=4, D=64, stream=None),
        "sage_merge_attn_states_multi_ex": dict(obs=blks, lbs=blks, count=3, dtype=0, oo=a, lo=a, rows=4, D=64, mult=1.0,
                                                corr=None, cmult=0.0, stream=None),
        "sage_merge_attn_states_multi": dict(obs=blks, lbs=blks, count=3, dtype=0, oo=a, lo=a, rows=4, D=64, stream=None),
        "sage_finish_lse": dict(l2=a, corr=None, sm=0.125, lo=a, n=64, stream=None),
        "sage_attn_qk_int8_pv_f16": attn,
        "sage_attn_qk_int8_pv_f8": attn,
        "sage_attn_qk_int8_pv_f16_varlen": dict(attn, cuq=a, cuk=a),
        "sage_attn_fusedq_pv_f16": dict(attn, qdt=0, km=a),
        "sage_attn_fusedq_pv_f8": dict(attn, qdt=0, km=a),
        "sage_attn_qk_int8_pv_f16_masked": dict(attn, mask=a, mkind=1, mstr=(C.c_int64 * 4)(0, 0, 64, 1)),
        "sage_attn_qk_int8_pv_f16_kvtiles": dict(attn, lay=L.KvLayout(0, 0, 0, 0, 0)),
        "sage_attn_qk_int8_pv_f8_kvtiles": dict(attn, lay=L.KvLayout(0, 0, 0, 0, 0)),
        "sage_sageattn_pv_f16": op,
        "sage_sageattn_pv_f8": op,
    }


def _call(fn, **change):
    from sageattention_amd import _lib as L
    args = dict(_valid_args()[fn], **change)
    return getattr(L.lib(), fn)(*[args[n] for n in _PARAMS[fn].split()])


def _single_faults():
    """(entry point, the one argument made invalid, expected status).  Each of these was already rejected before any launch
    before the entry points were split into check and launch, with the same status."""
    import ctypes as C
    from sageattention_amd import _lib as L
    t = _t()
    nul, odd, s4 = _t(data=0), _t(data=ODD), _t(sn=4)  # null data, unaligned data, a stride that is not a multiple of 8
    s8 = _t(sn=8)                                       # ... of 16
    bad = -1
    shape = [("B", 0), ("H", 0), ("N", 0)]
    dim = [("D", 96, -2), ("dtype", 7, bad)]

    def rows(fn, *cases):
        return [(fn, c[0], c[1], c[2] if len(c) > 2 else bad) for c in cases]

    out = []
    out += rows("sage_k_mean", ("k", None), ("k", nul), ("k", odd), ("k", s4), ("km", None), ("ws", None), *shape, *dim)
    quant = [("x", None), ("x", odd), ("x", s4), ("out", None), ("out", s4), ("scale", None), ("gran", 0), ("gran", 4),
             ("rounding", 2), ("blk", 32), ("warp", 8), ("warp", 48), ("mean", ODD), *dim]
    out += rows("sage_quant_qk_int8", *quant, *shape, ("dvec", FAKE), ("dot", FAKE))
    out += [("sage_quant_qk_int8", "dvec+dot", dict(dvec=FAKE, dot=FAKE, dgroup=0), bad),
            ("sage_quant_qk_int8", "dvec+dot", dict(dvec=FAKE, dot=FAKE, dgroup=2), bad),
            ("sage_quant_qk_int8", "dvec+dot", dict(dvec=ODD, dot=FAKE), bad),
            ("sage_quant_qk_int8", "blk+warp", dict(blk=64, warp=128), bad)]
    out += rows("sage_quant_qk_int8_varlen", *quant, ("cu", None), ("nseq", 0), ("H", 0), ("N", 0))
    out += rows("sage_sub_mean_f16", ("v", None), ("v", odd), ("v", s4), ("vm", None), ("vm", ODD), ("out", nul),
                ("out", s4), *shape, *dim)
    out += rows("sage_quant_k_int8_kvtiles", ("k", odd), ("out", s4), ("scale", None), ("sstr", None), ("tile", 0),
                ("tile", -4096), ("tile", 4100), ("sstr", (C.c_int64 * 3)(256, 256, 2)), ("gran", 2), ("gran", 0),
                ("rounding", 2), ("mean", ODD), *shape, *dim)
    out += rows("sage_k_smooth_quant", ("k", None), ("k", odd), ("k", s4), ("km", None), ("ws", None), ("gran", 2),
                ("gran", 0), *shape, *dim)
    out += rows("sage_kv_prepare_fp8", ("k", odd), ("v", None), ("v", s4), ("k8", odd), ("k8", s4), ("ks", None),
                ("km", None), ("v8", None), ("v8", s8), ("vs", None), ("ws", None), ("smax", 0.0), ("smax", float("nan")),
                ("gran", 2), ("gran", 4), ("rounding", 5), *shape, *dim)
    out += rows("sage_quant_v_fp8", ("v", None), ("v", odd), ("v", s4), ("v8", nul), ("v8", s8), ("vs", None),
                ("ws", None), ("smax", 0.0), ("smax", -1.0), *shape, *dim)
    out += rows("sage_seq_stats", ("x", None), ("x", odd), ("x", s4), ("stats", None), ("ws", None), *shape, *dim)
    out += rows("sage_kv_stats_reduce", ("parts", 0), ("BH", 0), ("n", 0), ("pstride", 191), ("kst", None),
                ("km", None), ("vs", None), ("vc", None), ("smax", 0.0), *dim)
    out += [("sage_kv_stats_reduce", "kst+vst", dict(kst=None, vst=None, km=None), bad)]
    out += rows("sage_quant_v_fp8_apply", ("v", None), ("v", s4), ("v8", odd), ("v8", s8), ("vc", None), ("tile", -64),
                ("tile", 24), *shape, *dim)
    merge = [("rows", 0), ("D", 96, -2), ("dtype", 7)]
    out += rows("sage_merge_attn_states", ("oa", None), ("oa", ODD), ("la", None), ("ob", None), ("ob", ODD),
                ("lb", None), *merge)
    blk = lambda i, v: (C.c_void_p * 16)(*[v if j == i else FAKE for j in range(16)])  # noqa: E731
    multi = [("obs", None), ("lbs", None), ("oo", None), ("oo", ODD), ("count", 0), ("count", 17), ("obs", blk(2, None)),
             ("obs", blk(1, ODD)), ("lbs", blk(0, None)), *merge]
    out += rows("sage_merge_attn_states_multi_ex", *multi, ("mult", 0.0), ("mult", float("nan")))
    out += rows("sage_merge_attn_states_multi", *multi)
    out += rows("sage_finish_lse", ("l2", None), ("lo", None), ("n", 0))
    attn = [("q", None), ("q", odd), ("q", s8), ("k", s8), ("o", _t(sn=2)), ("qs", None), ("ks", None), ("B", 0),
            ("Hq", 0), ("Hk", 0), ("Hk", 3), ("M", 0), ("N", 0), ("sm", 0.0), ("sm", float("nan")), ("sm", float("inf")),
            ("gran", 0), ("gran", 4), ("blkq", 32), ("warpq", 8), ("warpq", 48), ("odt", 7), ("D", 96, -2),
            ("N", 1 << 25, -4)]
    out += rows("sage_attn_qk_int8_pv_f16", *attn, ("v", s4), ("vdt", 7), ("vm", ODD))
    out += rows("sage_attn_qk_int8_pv_f8", *attn, ("v", s8), ("vs", None), ("vs", ODD), ("vm", ODD))
    out += rows("sage_attn_qk_int8_pv_f16_varlen", ("cuq", None), ("cuk", None), ("q", odd), ("D", 96, -2), ("vdt", 7))
    fused = [("qdt", 7), ("gran", 1, -3), ("km", ODD, -3), ("q", odd), ("q", s4), ("ks", None), ("sm", 0.0), ("o", nul),
             ("D", 96, -2), ("odt", 7)]
    out += rows("sage_attn_fusedq_pv_f16", *fused, ("v", s4), ("vdt", 7))
    out += rows("sage_attn_fusedq_pv_f8", *fused, ("v", s8), ("vs", None))
    out += rows("sage_attn_qk_int8_pv_f16_masked", ("mask", None), ("mkind", 0), ("mkind", 4), ("mstr", None),
                ("q", odd), ("sm", 0.0), ("D", 96, -2), ("vdt", 7))
    lay = lambda *s: L.KvLayout(*s)  # noqa: E731
    tiles = [("lay", None), ("lay", lay(-64, 0, 0, 0, 0)), ("lay", lay(0, -64, 0, 0, 0)), ("lay", lay(24, 0, 0, 0, 0)),
             ("lay", lay(0, 0, 8, 8, 2)), ("lay", lay(0, 0, 6, 6, 4)), ("lay", lay(0, 0, -4, 4, 4)), ("q", odd),
             ("D", 96, -2)]
    out += rows("sage_attn_qk_int8_pv_f16_kvtiles", *tiles, ("lay", lay(0, 4, 0, 0, 0)))
    out += rows("sage_attn_qk_int8_pv_f8_kvtiles", *tiles, ("lay", lay(0, 8, 0, 0, 0)), ("vs", None))
    opts = lambda *o: L.OpOpts(*o)  # noqa: E731
    op = [("q", None), ("k", None), ("v", None), ("o", None), ("opts", None), ("ws", None), ("ws", ODD), ("wsb", 4096),
          ("D", 96, -2), ("dtype", 7), ("B", 0), ("Hk", 0), ("Hk", 3), ("M", 0), ("N", 0), ("k", odd),
          ("opts", opts(3, 32, 0, -1, 0), -3), ("opts", opts(3, 32, 1, -1, 5)), ("opts", opts(1, 32, 1, -1, 0)),
          ("opts", opts(3, 64, 1, -1, 0))]
    out += rows("sage_sageattn_pv_f16", *op)
    out += rows("sage_sageattn_pv_f8", *op, ("smax", 0.0), ("v", odd))
    out += _window_rows()
    return [(fn, what, c if isinstance(c, dict) else {what: c}, st) for fn, what, c, st in out]


def _window_rows():
    """The 2^31-byte window of a (b, h_kv) slice is measured with the STRIDES (ceil(N/64) tiles of 64 * stride_n), not
    with N * D: 128K keys whose rows lie far apart -- a K or V slice of a packed QKV projection with many heads, an FP8 V
    image whose channel rows are 16 MiB apart -- cross it although N * D is 16 MiB.  Each limit is pinned from both
    sides: the largest stride below it reaches the launch (-5 where no GPU is visible), the next one is TOO_LARGE (-4)."""
    N = 1 << 17  # 2048 tiles (+ one tile of slack in the check): k8 crosses at stride_n = 16376 bytes, a 16-bit v at 8188 elements
    k_ok, k_big, k_qkv = _t(sn=16368), _t(sn=16384), _t(sn=3 * 64 * 128)
    v_ok, v_big, v_qkv = _t(sn=8184), _t(sn=8192), _t(sn=3 * 32 * 128)
    f8_ok, f8_big = _t(sn=(1 << 24) - 1040), _t(sn=(1 << 24) - 1024)  # D * stride_n + 64 * 2049 bytes
    out = []
    for fn, v_rows in (("sage_attn_qk_int8_pv_f16", (v_ok, v_big, v_qkv)), ("sage_attn_fusedq_pv_f16", (v_ok, v_big, v_qkv)),
                       ("sage_attn_qk_int8_pv_f8", (f8_ok, f8_big, None)), ("sage_attn_fusedq_pv_f8", (f8_ok, f8_big, None))):
        out += [(fn, "N", dict(N=N, D=128), -5),
                (fn, "k window", dict(N=N, D=128, k=k_ok), -5), (fn, "k window", dict(N=N, D=128, k=k_big), -4),
                (fn, "k window", dict(N=N, D=128, k=k_qkv), -4),
                (fn, "v window", dict(N=N, D=128, v=v_rows[0]), -5), (fn, "v window", dict(N=N, D=128, v=v_rows[1]), -4)]
        if v_rows[2] is not None:
            out.append((fn, "v window", dict(N=N, D=128, v=v_rows[2]), -4))
    # the one-call operators quantize K (and for FP8 PV also V) into dense workspace images: only the FP16-PV operator's v
    # reaches the attention kernel with the caller's strides
    fn = "sage_sageattn_pv_f16"
    out += [(fn, "N", dict(N=N, D=128), -5), (fn, "v window", dict(N=N, D=128, v=v_ok), -5),
            (fn, "v window", dict(N=N, D=128, v=v_big), -4), (fn, "v window", dict(N=N, D=128, v=v_qkv), -4),
            (fn, "k stride", dict(N=N, D=128, k=k_qkv), -5), ("sage_sageattn_pv_f8", "k, v strides", dict(N=N, D=128, k=v_qkv, v=v_qkv), -5)]
    return out


@no_gpu
def test_single_fault_status_table(built_lib):
    """Each argument made invalid on its own is rejected with its status."""
    cases = _single_faults()
    assert {fn for fn, *_ in cases} == set(_PARAMS)
    wrong = [(fn, what, st, got) for fn, what, change, st in cases if (got := _call(fn, **change)) != st]
    assert not wrong, wrong


@no_gpu
def test_rejected_before_any_launch(built_lib):
    """A call that returns an argument status has enqueued nothing: with no GPU every launch attempt fails, so a valid call
    returns SAGE_ERR_LAUNCH, and an invalid one must return its argument status instead."""
    from sageattention_amd import _lib as L
    not_launched = [fn for fn in _PARAMS if _call(fn) != -5]
    assert not not_launched, not_launched  # the control: every valid call reaches a launch
    fuse0 = L.OpOpts(3, 32, 1, 0, 0)  # the stand-alone Q quantizer
    cases = [("sage_k_smooth_quant", dict(out=_t(data=ODD))), ("sage_k_smooth_quant", dict(scale=None)),
             ("sage_k_smooth_quant", dict(rounding=5))]
    for fn in ("sage_sageattn_pv_f16", "sage_sageattn_pv_f8"):
        for change in (dict(q=_t(data=ODD)), dict(o=_t(data=ODD)), dict(sm=0.0), dict(sm=float("nan"))):
            cases += [(fn, change), (fn, dict(change, opts=fuse0))]
    cases += [("sage_sageattn_pv_f16", dict(v=_t(data=ODD))), ("sage_sageattn_pv_f16", dict(v=_t(data=ODD), opts=fuse0))]
    launched = [(fn, sorted(change), got) for fn, change in cases if (got := _call(fn, **change)) != -1]
    assert not launched, launched
