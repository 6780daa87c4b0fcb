"""Per-batch key lengths on the block-sparse and Sparge paths without a GPU: the six new symbols are declared, exported and
bound; every new entry point reaches a launch with valid arguments and refuses every single fault its twin refuses, with the
twin's status; the new custom ops exist beside the unchanged old ones; the Python keywords refuse what they must before any
device call.  What the kernels compute: test_sparse_kvlen_gpu.py."""
import ctypes
import inspect

import pytest
import torch

import test_kvlen as K  # _header_params: the parameter list of a declaration in include/sageattn_hip.h

ATTN = ["sage_attn_qk_int8_pv_f16_blocksparse", "sage_attn_qk_int8_pv_f8_blocksparse", "sage_attn_fusedq_pv_f16_blocksparse",
        "sage_attn_fusedq_pv_f8_blocksparse"]
PREDICTOR = ["sage_block_pool_sim", "sage_block_select"]
# new symbol -> its twin: the attention entry points take the arguments of the twin WITH the P.V skip
TWIN = {**{a + "_kvlen": a + "_pvskip" for a in ATTN}, **{p + "_kvlen": p for p in PREDICTOR}}


# ---- 1. the symbols --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TWIN))
def test_symbol_is_the_twin_plus_kv_lens(name):
    """declared with the twin's parameters and ``const int32_t* kv_lens`` in front of the stream; exported; bound alike"""
    from sageattention_amd import _build, _lib
    tp, kp = K._header_params(TWIN[name]), K._header_params(name)
    assert kp[:-2] == tp[:-1], (kp, tp)
    assert kp[-2] == ("const int32_t*", "kv_lens") and kp[-1] == tp[-1] == ("sage_stream_t", "stream")
    assert hasattr(ctypes.CDLL(_build.build()), name), f"{name} is not exported"
    (tres, targs), (kres, kargs) = _lib.SIGNATURES[TWIN[name]], _lib.SIGNATURES[name]
    assert kres is tres and kargs == targs[:-1] + [ctypes.c_void_p] + targs[-1:]
    assert len(kargs) == len(kp)


def test_abi_version_stays():
    from sageattention_amd import _build, _lib as L
    _build.build()
    assert L.lib().sage_abi_version() == 3


# ---- 2. every argument is checked before the first launch ------------------------------------------------------------------
# Fake device addresses: where a GPU is visible a missed check would launch kernels on them, so this runs only where none is;
# there every launch attempt returns SAGE_ERR_LAUNCH (-5), which makes a launch observable (tests/test_cabi_symbols.py).
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")
FAKE = 1 << 20
ODD4, ODD16 = FAKE + 2, FAKE + 8  # not 4-byte / not 16-byte aligned

_ATTN_PARAMS = {
    "sage_attn_qk_int8_pv_f16_blocksparse": "q k v vdt o odt qs ks vm lse B Hq Hk M N D causal gran blkq warpq sm lm1 lists lbytes",
    "sage_attn_qk_int8_pv_f8_blocksparse": "q k v o odt qs ks vs vm lse B Hq Hk M N D causal gran blkq warpq sm lm1 lists lbytes",
    "sage_attn_fusedq_pv_f16_blocksparse": "q qdt k v vdt o odt ks km vm lse B Hq Hk M N D causal gran warpq sm lists lbytes",
    "sage_attn_fusedq_pv_f8_blocksparse": "q qdt k v o odt ks km vs vm lse B Hq Hk M N D causal gran warpq sm lists lbytes",
}
_PARAMS = {}
for _a, _p in _ATTN_PARAMS.items():
    _PARAMS[_a + "_pvskip"] = _p + " thr skipped stream"
    _PARAMS[_a + "_kvlen"] = _p + " thr skipped lens stream"
_PARAMS["sage_block_pool_sim"] = "x dt B Hk N D blk mean pooled sim stream"
_PARAMS["sage_block_pool_sim_kvlen"] = "x dt B Hk N D blk mean pooled sim lens stream"
_SEL = "pq sq pk sk B Hq Hk M N D sm sthr rule par kf kl lists lbytes bmap"
_PARAMS["sage_block_select"] = _SEL + " stream"
_PARAMS["sage_block_select_kvlen"] = _SEL + " lens stream"


def _call(fn, **change):
    from sageattention_amd import _build, _lib as L
    _build.build()
    t = L.SageTensor(FAKE, 1 << 16, 1 << 12, 64)
    args = dict(q=t, k=t, v=t, o=t, x=t, dt=0, vdt=0, odt=0, qdt=0, qs=FAKE, ks=FAKE, vs=FAKE, vm=None, km=FAKE, lse=None,
                B=2, Hq=2, Hk=1, M=200, N=333, D=64, causal=0, gran=3, blkq=128, warpq=32, sm=0.125, lm1=0, lists=FAKE,
                lbytes=1 << 20, thr=FAKE, skipped=FAKE, lens=FAKE, stream=None, blk=64, mean=FAKE, pooled=FAKE, sim=FAKE,
                pq=FAKE, sq=FAKE, pk=FAKE, sk=FAKE, sthr=FAKE, rule=1, par=FAKE, kf=1, kl=2, bmap=FAKE)
    args.update(change)
    for key, value in list(args.items()):  # a tensor descriptor changed by field: q=dict(data=None)
        if isinstance(value, dict):
            base = dict(data=FAKE, stride_b=1 << 16, stride_h=1 << 12, stride_n=64)
            base.update(value)
            args[key] = L.SageTensor(base["data"], base["stride_b"], base["stride_h"], base["stride_n"])
    return getattr(L.lib(), fn)(*[args[n] for n in _PARAMS[fn].split()])


@no_gpu
def test_valid_calls_reach_a_launch():
    new = sorted(TWIN)
    assert [fn for fn in new if _call(fn) != -5] == []
    attn = [fn for fn in new if "attn" in fn]
    assert [fn for fn in attn if _call(fn, thr=None) != -5] == [], "pv_thresh == NULL selects the kernel without the skip"
    assert [fn for fn in attn if _call(fn, thr=None, skipped=None) != -5] == []
    assert [fn for fn in attn if _call(fn, skipped=None, lse=FAKE) != -5] == []
    assert [fn for fn in new if "block" in fn and "attn" not in fn and _call(fn, bmap=None, mean=None, rule=0, kf=0, kl=0) != -5] == []


# Single faults.  Each change is run through the twin AND the new entry point: the twin's status is the yardstick, and it must
# be an argument status (not 0, not -5: something was refused before a launch).  thr=None is left out on purpose: the twin
# refuses a NULL pv_thresh, while for the new entry points it is a valid argument that selects the kernel without the skip
# (include/sageattn_hip.h; covered by test_valid_calls_reach_a_launch).
_ATTN_FAULTS = [dict(thr=ODD4), dict(skipped=ODD4), dict(lists=None), dict(lists=ODD16), dict(lbytes=16), dict(causal=1),
                dict(vm=FAKE), dict(vm=ODD16), dict(D=96), dict(D=0), dict(B=0), dict(Hq=0), dict(Hk=0), dict(Hk=3), dict(M=0),
                dict(N=0), dict(ks=None), dict(sm=0.0), dict(sm=float("nan")), dict(gran=0), dict(gran=4), dict(warpq=48),
                dict(odt=2), dict(N=1 << 25, lbytes=1 << 40), dict(q=None), dict(k=None), dict(v=None), dict(o=None),
                dict(q=dict(data=None)), dict(k=dict(data=ODD16)), dict(v=dict(stride_n=3)), dict(o=dict(data=ODD4 + 1)),
                dict(causal=1, lists=None)]
_INT8_FAULTS = [dict(qs=None), dict(blkq=96), dict(vdt=2)]     # the forms with a pre-quantized Q (vdt: FP16 PV only)
_FUSED_FAULTS = [dict(qdt=2), dict(km=ODD16), dict(gran=1)]    # the forms with the fused Q quantizer
_FP8_FAULTS = [dict(vs=None), dict(vs=ODD16)]
_POOL_FAULTS = [dict(x=None), dict(x=dict(data=None)), dict(x=dict(stride_n=4)), dict(pooled=None), dict(pooled=ODD16),
                dict(sim=None), dict(mean=ODD16), dict(B=0), dict(Hk=0), dict(N=0), dict(D=96), dict(blk=32), dict(dt=2)]
_SELECT_FAULTS = [dict(pq=None), dict(sq=None), dict(pk=None), dict(sk=None), dict(sthr=None), dict(par=None), dict(lists=None),
                  dict(pq=ODD16), dict(pk=ODD16), dict(lists=ODD16), dict(B=0), dict(Hq=0), dict(Hk=0), dict(Hk=3), dict(M=0),
                  dict(N=0), dict(rule=2), dict(rule=-1), dict(kf=-1), dict(kl=-1), dict(D=96), dict(sm=0.0),
                  dict(sm=float("inf")), dict(N=64 * 2048 + 1, lbytes=1 << 40), dict(lbytes=16)]


def _faults(fn):
    if "pool" in fn:
        return _POOL_FAULTS
    if "select" in fn:
        return _SELECT_FAULTS
    out = list(_ATTN_FAULTS)
    out += _FUSED_FAULTS if "fusedq" in fn else _INT8_FAULTS
    if "_f8_" in fn:
        out = [f for f in out if "vdt" not in f] + _FP8_FAULTS
    return out


@no_gpu
@pytest.mark.parametrize("name", sorted(TWIN))
def test_single_faults_get_the_status_of_the_twin(name):
    wrong = []
    for change in _faults(name):
        want, got = _call(TWIN[name], **change), _call(name, **change)
        if want not in (-1, -2, -3, -4) or got != want:
            wrong.append((change, want, got))
    assert not wrong, wrong


@no_gpu
@pytest.mark.parametrize("name", sorted(TWIN))
def test_kv_lens_is_checked_before_any_launch(name):
    assert _call(name, lens=None) == -1 and _call(name, lens=ODD4) == -1  # SAGE_ERR_INVALID_ARGUMENT
    if "attn" in name:  # argument statuses come before the unsupported combinations, as the twin orders its checks
        assert _call(name, lens=None, causal=1) == -1 and _call(name, lens=None, thr=None) == -1


# ---- 3. the torch.library ops ----------------------------------------------------------------------------------------------
_T = "Tensor q, Tensor k, Tensor v, "
_TAIL = "Tensor kv_lens, str tensor_layout, float sm_scale, str pv, str qk_quant_gran)"
_SELECT = "Tensor simthreshd1, Tensor rule_param, str rule, SymInt keep_first, SymInt keep_last, "
NEW_SCHEMAS = {
    "attn_block_sparse_kvlen": "(" + _T + "Tensor block_map, " + _TAIL + " -> Tensor",
    "attn_block_sparse_plan_kvlen": "(" + _T + "Tensor block_lists, SymInt[] plan_shape, " + _TAIL + " -> Tensor",
    "attn_block_sparse_pv_kvlen": "(" + _T + "Tensor block_map, Tensor pvthreshd, " + _TAIL + " -> (Tensor, Tensor)",
    "attn_block_sparse_plan_pv_kvlen": "(" + _T + "Tensor block_lists, SymInt[] plan_shape, Tensor pvthreshd, " + _TAIL
                                       + " -> (Tensor, Tensor)",
    "attn_sparge_select_kvlen": "(" + _T + _SELECT + _TAIL + " -> Tensor",
    "attn_sparge_select_lse_kvlen": "(" + _T + _SELECT + _TAIL + " -> (Tensor, Tensor)",
    "attn_sparge_pv_kvlen": "(" + _T + _SELECT + "Tensor pvthreshd, " + _TAIL + " -> (Tensor, Tensor)",
    "attn_sparge_pv_lse_kvlen": "(" + _T + _SELECT + "Tensor pvthreshd, " + _TAIL + " -> (Tensor, Tensor, Tensor)",
}


def test_new_op_schemas_exist_and_the_old_ones_are_unchanged():
    import sageattention_amd.ops  # noqa: F401
    import test_pvskip as P
    for name, sig in {**P.OLD_SCHEMAS, **P.NEW_SCHEMAS, **NEW_SCHEMAS}.items():
        assert str(getattr(torch.ops.sageattention_amd, name).default._schema) == f"sageattention_amd::{name}{sig}"


def test_fake_shapes_in_both_layouts():
    """what torch.compile traces: every wrapper keyword combination, HND and NHD, head_dim 72"""
    import sageattention_amd.ops as ops
    from sageattention_amd import core
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        for layout, shp, kshp in (("HND", (3, 8, 300, 72), (3, 4, 333, 72)), ("NHD", (3, 300, 8, 72), (3, 333, 4, 72))):
            q = torch.empty(shp, dtype=torch.bfloat16, device="cuda")
            k = torch.empty(kshp, dtype=torch.bfloat16, device="cuda")
            lens = torch.empty((3,), dtype=torch.int32, device="cuda")
            bm = torch.empty((3, 8, 3, 6), dtype=torch.bool, device="cuda")
            plan = core.BlockSparsePlan(torch.empty(3 * 8 * 3 * 12, dtype=torch.int32, device="cuda"), 3, 8, 300, 333)
            for m in (bm, plan):
                o = ops.sageattn_block_sparse_compilable(q, k, k, m, tensor_layout=layout, pv="fp8", kv_lens=lens)
                assert o.shape == q.shape and o.dtype == q.dtype and o.is_contiguous()
                o, sk = ops.sageattn_block_sparse_compilable(q, k, k, m, tensor_layout=layout, pvthreshd=8.0, return_skipped=True,
                                                             kv_lens=lens)
                assert o.shape == q.shape and tuple(sk.shape) == (3, 8, 3, 4) and sk.dtype == torch.int32
                assert ops.sageattn_block_sparse_compilable(q, k, k, m, tensor_layout=layout, pvthreshd=8.0,
                                                            kv_lens=lens).shape == q.shape
            o = ops.sageattn_sparge_compilable(q, k, k, tensor_layout=layout, kv_lens=lens)
            assert o.shape == q.shape and o.is_contiguous()
            o, lse = ops.sageattn_sparge_compilable(q, k, k, tensor_layout=layout, topk=0.25, keep_last=2, return_lse=True,
                                                    kv_lens=lens)
            assert o.shape == q.shape and tuple(lse.shape) == (3, 8, 300) and lse.dtype == torch.float32
            o, sk = ops.sageattn_sparge_compilable(q, k, k, tensor_layout=layout, pvthreshd=8.0, return_skipped=True, kv_lens=lens)
            assert o.shape == q.shape and tuple(sk.shape) == (3, 8, 3, 4)
            o, lse, sk = ops.sageattn_sparge_compilable(q, k, k, tensor_layout=layout, pvthreshd=8.0, return_skipped=True,
                                                        return_lse=True, pv="fp8", kv_lens=lens)
            assert tuple(lse.shape) == (3, 8, 300) and tuple(sk.shape) == (3, 8, 3, 4)


# ---- 4. Python-level errors, raised before any device call -----------------------------------------------------------------
def test_keyword_exists_and_defaults_to_none():
    import sageattention_amd.ops as ops
    from sageattention_amd import core
    for fn in (core.sageattn_block_sparse, core.sageattn_sparge, core.sparge_plan, ops.sageattn_block_sparse_compilable,
               ops.sageattn_sparge_compilable):
        assert inspect.signature(fn).parameters["kv_lens"].default is None, fn


def test_python_errors():
    from sageattention_amd import core
    q = torch.zeros(2, 4, 200, 64, dtype=torch.float16)
    k = torch.zeros(2, 2, 320, 64, dtype=torch.float16)
    bm = torch.ones(2, 4, 2, 5, dtype=torch.bool)
    lens = torch.tensor([320, 7], dtype=torch.int32)
    calls = {"block_sparse": lambda **kw: core.sageattn_block_sparse(q, k, kw.pop("v", k), bm, **kw),
             "sparge": lambda **kw: core.sageattn_sparge(q, k, kw.pop("v", k), **kw),
             "plan": lambda **kw: core.sparge_plan(q, k, **kw)}
    for name, call in calls.items():
        for bad in (lens.long(), lens.float()):
            with pytest.raises(TypeError, match="int32"):
                call(kv_lens=bad)
        with pytest.raises(TypeError, match="kv_lens"):
            call(kv_lens=[320, 7])
        for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), torch.zeros((), dtype=torch.int32)):
            with pytest.raises(ValueError, match="kv_lens shape"):
                call(kv_lens=bad)
        with pytest.raises(ValueError, match="is on"):
            call(kv_lens=lens.to("meta"))
        with pytest.raises(AssertionError, match="cuda"):  # valid keywords: as every operator of the package on CPU tensors
            call(kv_lens=lens)
    with pytest.raises(ValueError, match="smooth_k"):
        calls["block_sparse"](kv_lens=lens, smooth_k=False)
    for name in ("block_sparse", "sparge"):
        with pytest.raises(ValueError, match="one shape"):
            calls[name](kv_lens=lens, pv="fp8", v=k[..., :32])
    with pytest.raises(ValueError, match="kv_lens shape"):  # the batch is the first axis in either layout
        core.sageattn_block_sparse(q.transpose(1, 2), k.transpose(1, 2), k.transpose(1, 2), bm, tensor_layout="NHD",
                                   kv_lens=torch.zeros(4, dtype=torch.int32))


def test_out_of_scope_operators_refuse_the_keyword():
    """sageattn_tile_mass, plan_recall and sparge_tune keep their signatures (tests/test_calib.py pins them): kv_lens is an
    unknown keyword there, a TypeError before anything runs, and their docstrings say that lengths are not built"""
    from sageattention_amd import core
    q = torch.zeros(1, 1, 128, 64, dtype=torch.float16)
    lens = torch.tensor([64], dtype=torch.int32)
    with pytest.raises(TypeError, match="kv_lens"):
        core.sageattn_tile_mass(q, q, kv_lens=lens)
    with pytest.raises(TypeError, match="kv_lens"):
        core.plan_recall(torch.ones(1, 1, 1, 2, dtype=torch.bool), torch.zeros(1, 1, 1, 2), kv_lens=lens)
    with pytest.raises(TypeError, match="kv_lens"):
        core.sparge_tune(q, q, kv_lens=lens)
    for fn in (core.sageattn_tile_mass, core.plan_recall, core.sparge_tune):
        assert "kv_lens" in fn.__doc__ and "kv_lens" not in inspect.signature(fn).parameters
    with pytest.raises(TypeError):  # query lengths and a causal form are not built: no such keywords
        core.sageattn_block_sparse(q, q, q, torch.ones(1, 1, 1, 2, dtype=torch.bool), q_lens=lens)
    with pytest.raises(ValueError, match="non-causal"):
        core.sageattn_block_sparse(q, q, q, torch.ones(1, 1, 1, 2, dtype=torch.bool), kv_lens=lens, is_causal=True)
