"""The MXFP4 V image of the KV cache (sageattention_amd/fp4.py) without a GPU: the new header against its ctypes table, the
ops of the new namespace, and the refusals of the Python layer.  What the kernels compute: test_fp4_gpu.py."""
import os
import re

import pytest
import torch

import sageattention_amd as sa
from sageattention_amd import _lib as L
from sageattention_amd import fp4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("quant_v_mxfp4", "kv_cache_append_v4", "attn_splitkv_v4", "attn_splitkv_v4_lse", "attn_splitkv_causal_v4",
       "attn_splitkv_causal_v4_lse")


def test_header_and_table_agree():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "sageattn_hip_fp4.h")).read(), flags=re.S)
    protos = {name: len(params.split(",")) for name, params in re.findall(r"\b(sage_\w+)\s*\(([^()]*)\)\s*;", text)}
    assert protos == {name: len(args) for name, (_, args) in L.FP4_SIGNATURES.items()} and len(protos) == 4
    lib = L.lib()
    assert all(getattr(lib, name).argtypes == args for name, (_, args) in L.FP4_SIGNATURES.items())


def test_ops_are_registered_in_their_own_namespace():
    names = torch._C._dispatch_get_all_op_names()
    assert all(f"sageattention_amd_fp4::{n}" in names for n in OPS)
    assert {"quant_v_mxfp4", "SageKVCacheV4", "sageattn_splitkv_v4"} <= set(sa.__all__)
    schema = str(torch.ops.sageattention_amd_fp4.kv_cache_append_v4.default._schema)
    assert all(re.search(rf"Tensor\(\w+!\) {n}\b", schema) for n in ("k8", "k_scale", "v4", "v4_scale"))


@pytest.mark.parametrize("shape,dtype,layout,err", [
    ((1, 1, 64, 96), torch.float16, "HND", "head_dim 64 or 128"),
    ((1, 1, 64, 64), torch.float32, "HND", "fp16 or bf16"),
    ((1, 64, 64), torch.float16, "HND", "4-D"),
    ((1, 1, 64, 64), torch.float16, "DNH", "Unknown tensor layout"),
])
def test_quantizer_refuses(shape, dtype, layout, err):
    with pytest.raises(ValueError, match=err):
        fp4.quant_v_mxfp4(torch.zeros(shape, dtype=dtype), None, layout)


def test_quantizer_refuses_wrong_buffers_and_lengths():
    v = torch.zeros(2, 1, 70, 64, dtype=torch.float16)
    with pytest.raises(TypeError, match="int32"):
        fp4.quant_v_mxfp4(v, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"img must be a contiguous uint8 tensor of shape \(2, 1, 64, 64\)"):
        fp4.quant_v_mxfp4(v, None, "HND", out=(torch.zeros(2, 1, 64, 32, dtype=torch.uint8), torch.zeros(2, 1, 2, 128, dtype=torch.uint8)))


@pytest.mark.parametrize("status,args", [
    (-1, dict(scale=0)), (-1, dict(scale=8)), (-1, dict(img=8)), (-1, dict(B=0)), (-1, dict(kv_lens=2)), (-2, dict(D=96))])
def test_c_entry_checks_before_any_launch(status, args):
    """sage_quant_v_mxfp4 on made-up aligned addresses: an argument status comes back before anything is dereferenced"""
    a = dict(img=4096, scale=8192, B=1, D=64, kv_lens=0) | args
    t = L.SageTensor(1 << 20, 64 * 64, 64 * 64, 64)
    img = L.SageTensor(a["img"], 64 * 32, 64 * 32, 32)
    assert L.lib().sage_quant_v_mxfp4(t, 0, a["B"], 1, 64, a["D"], img, a["scale"] or None, a["kv_lens"] or None, None) == status


def test_attention_refuses_what_the_cached_operator_refuses():
    q = torch.zeros(1, 1, 4, 64, dtype=torch.float16)
    with pytest.raises(TypeError, match="SageKVCacheV4"):
        sa.sageattn_splitkv_v4(q, object())
    kc = sa.SageKVCache(q, q, "fp16", "per_thread", "HND", 2.0)
    cache = sa.SageKVCacheV4(kc, None, None)
    for kw, exc in ((dict(attn_mask=q), ValueError), (dict(smooth_k=False), ValueError), (dict(pv="fp8"), TypeError),
                    (dict(num_splits=17), ValueError), (dict(q_fold=3, causal=True), ValueError), (dict(q_fold=2), ValueError)):
        with pytest.raises(exc):
            sa.sageattn_splitkv_v4(q, cache, **kw)
    with pytest.raises(ValueError, match="max_new"):
        cache.append(None, None, 0)
