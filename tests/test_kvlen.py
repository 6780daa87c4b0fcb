"""Per-batch key lengths (``sageattn_kvlen``, the ``*_kvlen`` entry points) without a GPU: the six symbols are declared,
exported and bound as their twins plus one pointer, the argument checks return their status before any launch, the op
schemas and fake kernels, and the Python-level errors.  What the kernels compute: test_kvlen_gpu.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TWINS = ["sage_k_smooth_quant", "sage_kv_prepare_fp8", "sage_attn_qk_int8_pv_f16", "sage_attn_qk_int8_pv_f8",
         "sage_attn_fusedq_pv_f16", "sage_attn_fusedq_pv_f8"]


# ---- 1. the six symbols ---------------------------------------------------------------------------------------------------
def _header_params(name):
    """the parameter list of ``name`` in include/sageattn_hip.h, as (type, name) pairs"""
    text = open(os.path.join(ROOT, "include", "sageattn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/sageattn_hip.h"
    out = []
    for par in m.group(1).split(","):
        par = " ".join(par.split())
        out.append(tuple(par.rsplit(" ", 1)))
    return out


@pytest.mark.parametrize("twin", TWINS)
def test_symbol_is_the_twin_plus_kv_lens(twin):
    """declared with the twin's parameters and ``const int32_t* kv_lens`` in front of the stream; exported; bound alike"""
    from sageattention_amd import _build, _lib
    name = twin + "_kvlen"
    tp, kp = _header_params(twin), _header_params(name)
    assert kp[:-2] == tp[:-1], (kp, tp)
    assert kp[-2] == ("const int32_t*", "kv_lens") and kp[-1] == tp[-1] == ("sage_stream_t", "stream")
    assert hasattr(ctypes.CDLL(_build.build()), name), f"{name} is not exported"
    (tres, targs), (kres, kargs) = _lib.SIGNATURES[twin], _lib.SIGNATURES[name]
    assert kres is tres and kargs == targs[:-1] + [ctypes.c_void_p] + targs[-1:]
    assert len(kargs) == len(kp)


# ---- 2. every argument is checked before the first launch ------------------------------------------------------------------
# Fake device addresses: where a GPU is visible a missed check would launch kernels on them, so this runs only where none
# is; there every launch attempt returns SAGE_ERR_LAUNCH (-5), which makes a launch observable (tests/test_cabi_symbols.py).
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")

FAKE = 1 << 20
ODD = FAKE + 2  # not 4-byte aligned

_PARAMS = {
    "sage_k_smooth_quant_kvlen": "k dt B Hk N D k8 ks km gran rnd ws lens stream",
    "sage_kv_prepare_fp8_kvlen": "k v dt B Hk N D k8 ks km gran rnd v8 vs smax ws lens stream",
    "sage_attn_qk_int8_pv_f16_kvlen": "q k v vdt o odt qs ks vm lse B Hq Hk M N D causal gran blkq warpq sm lm1 lens stream",
    "sage_attn_qk_int8_pv_f8_kvlen": "q k v o odt qs ks vs vm lse B Hq Hk M N D causal gran blkq warpq sm lm1 lens stream",
    "sage_attn_fusedq_pv_f16_kvlen": "q qdt k v vdt o odt ks km vm lse B Hq Hk M N D causal gran warpq sm lens stream",
    "sage_attn_fusedq_pv_f8_kvlen": "q qdt k v o odt ks km vs vm lse B Hq Hk M N D causal gran warpq sm lens stream",
}


def _call(fn, **change):
    from sageattention_amd import _lib as L
    t = L.SageTensor(FAKE, 1 << 16, 1 << 12, 64)
    args = dict(q=t, k=t, v=t, o=t, k8=t, v8=t, dt=0, vdt=0, odt=0, qdt=0, qs=FAKE, ks=FAKE, vs=FAKE, vm=None, km=FAKE, lse=None,
                B=2, Hq=2, Hk=1, M=200, N=333, D=64, causal=0, gran=3, rnd=0, blkq=128, warpq=32, sm=0.125, lm1=0, smax=448.0,
                ws=FAKE, lens=FAKE, stream=None)
    args.update(change)
    return getattr(L.lib(), fn)(*[args[n] for n in _PARAMS[fn].split()])


@no_gpu
def test_valid_calls_reach_a_launch():
    assert [fn for fn in _PARAMS if _call(fn) != -5] == []
    assert [fn for fn in _PARAMS if "attn" in fn and _call(fn, causal=1, lse=FAKE) != -5] == []


@no_gpu
def test_status_table():
    """Each argument made invalid on its own returns its argument status: nothing was launched (a launch returns -5 here)."""
    cases = []
    for fn in _PARAMS:
        cases += [(fn, dict(lens=None), -1), (fn, dict(lens=ODD), -1), (fn, dict(D=96), -2), (fn, dict(N=0), -1),
                  (fn, dict(B=0), -1), (fn, dict(ks=None), -1)]
    for fn in (f for f in _PARAMS if "attn" in f):
        cases += [(fn, dict(sm=0.0), -1), (fn, dict(Hk=3), -1), (fn, dict(N=1 << 25), -4)]
    for fn in (f for f in _PARAMS if "attn" not in f):
        cases += [(fn, dict(km=None), -1), (fn, dict(km=FAKE + 8), -1), (fn, dict(ws=None), -1), (fn, dict(gran=2), -1)]
    wrong = [(fn, sorted(c), st, got) for fn, c, st in cases if (got := _call(fn, **c)) != st]
    assert not wrong, wrong


def test_kv_lens_with_the_forms_not_built(tmp_path):
    """attn_check refuses kv_lens together with tile lists, an attn_mask, cu_seqlens or a tile layout with
    SAGE_ERR_UNSUPPORTED (-3).  The C ABI has no entry point with both, so a host-only probe (kvlen_check_probe.cpp) fills
    the host layer's argument block and calls the check of the built library; the check makes no HIP call."""
    from sageattention_amd import _build
    lib = _build.build()
    exe = str(tmp_path / "kvlen_check_probe")
    libdir = os.path.dirname(lib)
    subprocess.run([_build.HIPCC, "-std=c++17", "-O0", "-x", "hip", "--offload-host-only", "-I", _build.CSRC,
                    os.path.join(ROOT, "tests", "kvlen_check_probe.cpp"), "-x", "none", lib, f"-Wl,-rpath,{libdir}", "-o", exe],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    got = dict((a, int(b)) for a, b in (line.split() for line in out.splitlines()))
    assert got == {"alone": 0, "lists": -3, "mask": -3, "cu_seqlens": -3, "layout": -3, "null": -1, "misaligned": -1}


# ---- 3. the torch.library ops ----------------------------------------------------------------------------------------------
def test_op_schemas_and_fake_shapes():
    import sageattention_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    want = ("Tensor q, Tensor k, Tensor v, Tensor kv_lens, str tensor_layout, bool is_causal, float sm_scale, str pv, "
            "str qk_quant_gran")
    s, s_lse = (str(getattr(torch.ops.sageattention_amd, n).default._schema) for n in ("attn_kvlen", "attn_kvlen_lse"))
    assert want in s and s.endswith("-> Tensor")
    assert want in s_lse and s_lse.endswith("-> (Tensor, Tensor)")
    assert "sageattn_kvlen_compilable" in ops.__all__
    with FakeTensorMode():
        for layout, shp, kshp in (("HND", (3, 8, 300, 72), (3, 4, 333, 72)), ("NHD", (3, 300, 8, 72), (3, 333, 4, 72))):
            q = torch.empty(shp, dtype=torch.bfloat16, device="cuda")
            k = torch.empty(kshp, dtype=torch.bfloat16, device="cuda")
            lens = torch.empty((3,), dtype=torch.int32, device="cuda")
            o = ops.sageattn_kvlen_compilable(q, k, k, lens, tensor_layout=layout, pv="fp8")
            assert o.shape == q.shape and o.dtype == q.dtype and o.device == q.device and o.is_contiguous()
            o, lse = ops.sageattn_kvlen_compilable(q, k, k, lens, tensor_layout=layout, is_causal=True, return_lse=True)
            assert o.shape == q.shape and lse.shape == (3, 8, 300) and lse.dtype == torch.float32
    with pytest.raises(ValueError, match="layout"):
        ops.sageattn_kvlen_compilable(torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64),
                                      torch.zeros(1, dtype=torch.int32), tensor_layout="BHSD")


# ---- 4. Python-level errors, raised before any device call -----------------------------------------------------------------
def test_python_errors():
    import sageattention_amd as sa
    from sageattention_amd import core
    assert "sageattn_kvlen" in sa.__all__ and "sageattn_kvlen" in core.__all__ and sa.sageattn_kvlen is core.sageattn_kvlen
    q = torch.zeros(2, 4, 200, 64, dtype=torch.float16)
    k = torch.zeros(2, 2, 320, 64, dtype=torch.float16)
    lens = torch.tensor([320, 7], dtype=torch.int32)
    with pytest.raises(TypeError, match="int32"):
        sa.sageattn_kvlen(q, k, k, lens.long())
    with pytest.raises(TypeError, match="int32"):
        sa.sageattn_kvlen(q, k, k, lens.float())
    with pytest.raises(TypeError, match="kv_lens"):
        sa.sageattn_kvlen(q, k, k, [320, 7])
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), torch.zeros((), dtype=torch.int32)):
        with pytest.raises(ValueError, match="kv_lens shape"):
            sa.sageattn_kvlen(q, k, k, bad)
    with pytest.raises(ValueError, match="kv_lens shape"):  # the batch is the first axis in either layout
        sa.sageattn_kvlen(q.transpose(1, 2), k.transpose(1, 2), k.transpose(1, 2), torch.zeros(4, dtype=torch.int32),
                          tensor_layout="NHD")
    with pytest.raises(ValueError, match="is on"):
        sa.sageattn_kvlen(q, k, k, lens.to("meta"))
    with pytest.raises(ValueError, match="pv"):
        sa.sageattn_kvlen(q, k, k, lens, pv="auto")
    with pytest.raises(ValueError, match="qk_quant_gran"):
        sa.sageattn_kvlen(q, k, k, lens, qk_quant_gran="per_block")
    with pytest.raises(ValueError, match="layout"):
        sa.sageattn_kvlen(q, k, k, lens, tensor_layout="BHSD")
    with pytest.raises(ValueError, match="one shape"):
        sa.sageattn_kvlen(q, k, k[..., :32], lens, pv="fp8")
    for kw in (dict(smooth_k=False), dict(smooth_v=True), dict(attn_mask=None)):  # not built: unknown keywords are not swallowed
        with pytest.raises(TypeError):
            sa.sageattn_kvlen(q, k, k, lens, **kw)
    with pytest.raises(AssertionError, match="cuda"):  # as every operator of the package on CPU tensors
        sa.sageattn_kvlen(q, k, k, lens)
