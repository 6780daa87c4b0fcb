"""The paged MXFP4 V cache (sageattention_amd/paged_fp4.py) without a GPU: the new header against its ctypes table, the ops of
the new namespace, and the refusals, which are those of ``sageattn_splitkv_paged``.  What the kernels compute:
test_paged_fp4_gpu.py."""
import os
import re

import pytest
import torch

import sageattention_amd as sa
from sageattention_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("kv_cache_append_paged_v4", "attn_splitkv_paged_v4", "attn_splitkv_paged_v4_lse", "attn_splitkv_causal_paged_v4",
       "attn_splitkv_causal_paged_v4_lse")


def test_header_and_table_agree():
    """(the causal and the non-causal form share one attention entry, so the header declares two symbols)"""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "sageattn_hip_paged_fp4.h")).read(), flags=re.S)
    protos = {name: len(params.split(",")) for name, params in re.findall(r"\b(sage_\w+)\s*\(([^()]*)\)\s*;", text)}
    assert protos == {name: len(args) for name, (_, args) in L.PAGED_FP4_SIGNATURES.items()}
    assert sorted(protos) == ["sage_attn_fusedq_pv_f4_splitkv_paged", "sage_kv_cache_append_paged_v4"]
    lib = L.lib()
    assert all(getattr(lib, name).argtypes == args for name, (_, args) in L.PAGED_FP4_SIGNATURES.items())


def test_ops_are_registered_in_their_own_namespace():
    names = torch._C._dispatch_get_all_op_names()
    assert all(f"sageattention_amd_paged_fp4::{n}" in names for n in OPS)
    assert {"SagePagedKVCacheV4", "sageattn_splitkv_paged_v4"} <= set(sa.__all__)
    schema = str(torch.ops.sageattention_amd_paged_fp4.kv_cache_append_paged_v4.default._schema)
    assert all(re.search(rf"Tensor\(\w+!\) {n}\b", schema) for n in ("k8", "k_scale", "v4", "v4_scale"))
    assert "block_table" in str(torch.ops.sageattention_amd_paged_fp4.attn_splitkv_causal_paged_v4_lse.default._schema)


def _raised(fn, *args, **kw):
    with pytest.raises((TypeError, ValueError)) as e:
        fn(*args, **kw)
    return type(e.value), str(e.value)


@pytest.mark.parametrize("bad", [dict(block_table=torch.zeros(1, 2, dtype=torch.int64)), dict(q_fold=3, causal=True),
                                 dict(q_fold=2), dict(num_splits=17), dict(attn_mask=True), dict(kv_lens=None)])
def test_attention_refuses_what_the_paged_operator_refuses(bad):
    q = torch.zeros(1, 1, 4, 64, dtype=torch.float16)
    k8 = sa.SagePagedKVCache(q, q, "fp8", "per_thread", "HND", 2.0)
    k4 = sa.SagePagedKVCacheV4(sa.SagePagedKVCache(q, q, "fp16", "per_thread", "HND", 2.0), None, None)
    args = dict(block_table=torch.zeros(1, 2, dtype=torch.int32), kv_lens=torch.zeros(1, dtype=torch.int32)) | bad
    assert _raised(sa.sageattn_splitkv_paged_v4, q, k4, **args) == _raised(sa.sageattn_splitkv_paged, q, k8, **args)


def test_cache_refusals():
    q = torch.zeros(1, 1, 4, 64, dtype=torch.float16)
    with pytest.raises(TypeError, match="SagePagedKVCacheV4"):  # the FP8 / FP16 paged cache is not this one
        sa.sageattn_splitkv_paged_v4(q, sa.SagePagedKVCache(q, q, "fp8", "per_thread", "HND", 2.0), None, None)
    pool, table, lens = torch.zeros(2, 1, 96, 64, dtype=torch.float16), torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    exc, msg = _raised(sa.SagePagedKVCacheV4.prepare, pool, pool, table, lens)  # a page of 96 keys
    assert exc is ValueError and "page_size must be 64, 128 or 256" in msg
    assert (exc, msg) == _raised(sa.SagePagedKVCache.prepare, pool, pool, table, lens)
    cache = sa.SagePagedKVCacheV4(sa.SagePagedKVCache(q, q, "fp16", "per_thread", "HND", 2.0), None, None)
    with pytest.raises(ValueError, match="max_new"):
        cache.append(table, lens, lens, 0)


@pytest.mark.parametrize("status,args", [(-1, dict(page_size=96)), (-1, dict(scale=0)), (-1, dict(scale=8)), (-1, dict(table=2)),
                                         (-1, dict(img_row=16)), (-2, dict(D=96)), (-1, dict(max_new=0))])
def test_c_append_checks_before_any_launch(status, args):
    """sage_kv_cache_append_paged_v4 on made-up aligned addresses: an argument status comes back before anything is dereferenced"""
    a = dict(page_size=64, scale=8192, table=4096, img_row=32, D=64, max_new=1) | args
    t = L.SageTensor(1 << 20, 64 * 64, 64 * 64, 64)
    img = L.SageTensor(1 << 22, 64 * a["img_row"], 64 * a["img_row"], a["img_row"])
    assert L.lib().sage_kv_cache_append_paged_v4(t, t, 0, 1, 1, a["D"], 1 << 16, t, 1 << 18, 3, 0, img, a["scale"] or None,
                                                 a["table"], 1, 1, a["page_size"], 2, 1 << 12, 1 << 13, a["max_new"], None) == status
