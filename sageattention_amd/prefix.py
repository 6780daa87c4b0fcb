"""Shared-prefix attention on the paged quantized KV cache: a batch whose sequences begin with the same system prompt or
few-shot header keeps ONE quantized copy of those pages and reads them from HBM once per step for the whole batch
(include/sageattn_hip_prefix.h holds the rule).

The frozen statistics -- the smoothing vector ``km`` and the FP8 V scale -- are per sequence, so a page's quantized bytes
belong to one sequence and several table rows cannot simply name it.  Here the prefix is a sequence of its own with its own
statistics, each suffix keeps its own, and a row's attention over prefix plus suffix is the log-sum-exp merge of two partial
attentions: the paged non-causal split-KV kernel on the prefix, with the B sequences' query rows folded into the rows of one
batch, the paged causal kernel on the suffixes as it stands, and one merge kernel that gives each segment its own ``q . km``
correction before it combines them.  For B sequences behind a prefix of Np keys and suffixes of Ns keys the K / V rows read
per step fall from B * (Np + Ns) to Np + B * Ns.

The intended use is one cache of B + 1 sequences, ``whole.narrow(0, 1)`` as the prefix and ``whole.narrow(1, B)`` as the
suffixes: ``prepare_`` and ``append`` / ``append_rows`` need no change.  Tables and lengths are read on the device only, so
{append; attention} captures into one HIP graph.  The ops live in a namespace of their own,
``torch.ops.sageattention_amd_prefix``: ``attn_splitkv_paged_prefix[_lse]``; they trace under ``torch.compile(fullgraph=True)``.

Not built: more than one prefix per call or trees of prefixes, one fused launch over both segments, the two attention
launches on two streams, prefix sharing for the contiguous ``SageKVCache``, and moving frozen statistics without preparing
again."""
from typing import Optional

import torch

from . import _lib as L
from . import core
from . import paged

__all__ = ["sageattn_splitkv_paged_prefix"]

_NS = "sageattention_amd_prefix"


def _foldable(q, tensor_layout):
    """can the C ABI address q [B,Hq,M,D] as it is, AND the folded view q_p[0, h, b * M + m] = q[b, h, m] with one row
    stride?  (NHD-contiguous q, any q with M = 1 or B = 1, and their slices along the last dim)"""
    if core._abi_view(q) is not q:
        return False
    B, _, M, _ = L.dims(q, tensor_layout)
    stride_b, stride_n = q.stride(0), q.stride(2 if tensor_layout == "HND" else 1)
    return B == 1 or M == 1 or stride_b == M * stride_n


def _prefix_attn(q, k8, k_scale, km, v, v_scale, block_table, kv_lens, prefix_table, prefix_len, km_p, v_scale_p, num_splits,
                 prefix_splits, q_fold, tensor_layout, sm_scale, qk_quant_gran, with_lse, workspace=None):
    """sage_attn_fusedq_pv_{f16,f8}_splitkv_paged_prefix on the pools two caches share (``v``: the fp16 / bf16 V pool, or with
    ``v_scale`` / ``v_scale_p`` the pool of V^T images): the workspace and the three launches.  num_splits / prefix_splits 0 =
    ``core.splitkv_num_splits`` on the segment's shape and logical capacity.  ``workspace`` (uint8, on q's device) is the
    caller's where given.  -> (o contiguous in q's shape, lse or None)"""
    B, Hq, M, D = L.dims(q, tensor_layout)
    P, Hk, page_size, _ = L.dims(k8, tensor_layout)
    num_splits = num_splits or core.splitkv_num_splits(B, Hq, M, block_table.size(1) * page_size)
    prefix_splits = prefix_splits or core.splitkv_num_splits(1, Hq, B * M, prefix_table.numel() * page_size)
    lib = L.lib()
    pv_fp8 = v_scale is not None
    with torch.cuda.device(q.device):
        if not _foldable(q, tensor_layout):
            # one copy, in the NHD memory order: the C ABI can address it and its folded view has one row stride
            q = q.contiguous() if tensor_layout == "NHD" else q.transpose(1, 2).contiguous().transpose(1, 2)
        o = torch.empty(q.size(), dtype=q.dtype, device=q.device)
        lse = torch.empty((B, Hq, M), dtype=torch.float32, device=q.device) if with_lse else None
        nbytes = lib.sage_prefix_workspace_bytes(B, Hq, M, D, prefix_splits, num_splits)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device) if workspace is None else workspace
        fn = f"sage_attn_fusedq_pv_{'f8' if pv_fp8 else 'f16'}_splitkv_paged_prefix"
        # in the order of the C signatures: the f8 form has no v_dtype and takes v_scale and v_scale_p
        v_args = (L.desc_vt(v, tensor_layout),) if pv_fp8 else (L.desc(v, tensor_layout), L.dtype_code(v.dtype))
        L.check(getattr(lib, fn)(
            L.desc(q, tensor_layout), L.dtype_code(q.dtype), L.desc(k8, tensor_layout), *v_args, L.desc(o, tensor_layout),
            L.dtype_code(o.dtype), k_scale.data_ptr(), km.data_ptr(), *((v_scale.data_ptr(),) if pv_fp8 else ()), L.ptr(lse),
            B, Hq, Hk, M, D, core._GRAN_CODE[qk_quant_gran], 32, float(sm_scale),
            *paged._table_args(block_table, page_size, P), kv_lens.data_ptr(), prefix_table.data_ptr(),
            prefix_table.numel(), prefix_len.data_ptr(), km_p.data_ptr(), *((v_scale_p.data_ptr(),) if pv_fp8 else ()),
            prefix_splits, num_splits, int(q_fold), ws.data_ptr(), ws.numel(), L.stream_ptr(q.device)), fn)
    return o, lse


def _register(name, with_lse):
    """attn_splitkv_paged_prefix[_lse]: ``_prefix_attn`` as an op; nothing is mutated"""
    params = ("Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor block_table, Tensor kv_lens, "
              "Tensor prefix_table, Tensor prefix_len, Tensor km_p, Tensor? v_scale_p, SymInt num_splits, SymInt prefix_splits, "
              "SymInt q_fold, str tensor_layout, float sm_scale, str qk_quant_gran")

    def body(*args):
        o, lse = _prefix_attn(*args, with_lse)
        return (o, lse) if with_lse else o

    def fake(q, k8, k_scale, km, v, v_scale, block_table, kv_lens, prefix_table, prefix_len, km_p, v_scale_p, num_splits,
             prefix_splits, q_fold, tensor_layout, sm_scale, qk_quant_gran):
        o = q.new_empty(q.shape)
        if not with_lse:
            return o
        B, Hq, M, _ = L.dims(q, tensor_layout)
        return o, q.new_empty((B, Hq, M), dtype=torch.float32)

    op = torch.library.custom_op(f"{_NS}::{name}", body, mutates_args=(),
                                 schema=f"({params}) -> {'(Tensor, Tensor)' if with_lse else 'Tensor'}")
    op.register_fake(fake)
    return op


attn_splitkv_paged_prefix = _register("attn_splitkv_paged_prefix", False)
attn_splitkv_paged_prefix_lse = _register("attn_splitkv_paged_prefix_lse", True)


def _v_pool(cache):
    """the fp16 / bf16 V pool the attention kernels read with FP16 / BF16 P.V (None with FP8 P.V for a cache that owns its pools)"""
    return cache.v if isinstance(cache, paged.SagePagedKVCache) else cache.v_pool


def _check_shared_pools(cache, prefix):
    """the two caches must be views of ONE set of pools, quantized alike; each mismatch is refused by name"""
    for name in ("pv", "qk_quant_gran", "tensor_layout", "dtype", "page_size"):
        a, b = getattr(cache, name), getattr(prefix, name)
        if a != b:
            raise ValueError(f"cache and prefix must share pools: {name} is {a!r} for cache and {b!r} for prefix")
    pools = [("k8", cache.k8, prefix.k8), ("k_scale", cache.k_scale, prefix.k_scale)]
    pools.append(("v8", cache.v8, prefix.v8) if cache.pv == "fp8" else ("v", _v_pool(cache), _v_pool(prefix)))
    for name, a, b in pools:
        if a is b:  # (narrow() hands the pools on as they are)
            continue
        if a is None or b is None or a.shape != b.shape or a.stride() != b.stride() or a.data_ptr() != b.data_ptr():
            raise ValueError(f"cache and prefix must share pools: their {name} pools differ (data_ptr, shape or strides); "
                             "take both from one cache with narrow()")


def _check_prefix_table(prefix_table, device):
    """``prefix_table`` as the kernels read it: int32 [max_prefix_pages >= 1] (or its [1, max_prefix_pages] row) on the device,
    contiguous; its values stay on the device"""
    if not isinstance(prefix_table, torch.Tensor):
        raise TypeError("prefix_table must be an int32 tensor of shape [max_prefix_pages]")
    if prefix_table.dtype != torch.int32:
        raise TypeError(f"prefix_table must be of dtype int32, got {prefix_table.dtype}")
    if prefix_table.dim() == 2 and prefix_table.size(0) == 1:
        prefix_table = prefix_table[0]
    if prefix_table.dim() != 1 or prefix_table.size(0) < 1:
        raise ValueError(f"prefix_table shape {tuple(prefix_table.shape)} does not match [max_prefix_pages >= 1]")
    if prefix_table.device != device:
        raise ValueError(f"prefix_table is on {prefix_table.device}, the pools on {device}")
    if prefix_table.stride(0) != 1:
        raise ValueError("prefix_table must be contiguous (stride(-1) == 1)")
    return prefix_table


def _check_prefix_len(prefix_len, device):
    if not isinstance(prefix_len, torch.Tensor):
        raise TypeError("prefix_len must be an int32 tensor of shape [1]")
    if prefix_len.dtype != torch.int32:
        raise TypeError(f"prefix_len must be of dtype int32, got {prefix_len.dtype}")
    if tuple(prefix_len.shape) != (1,):
        raise ValueError(f"prefix_len shape {tuple(prefix_len.shape)} does not match [1]")
    if prefix_len.device != device:
        raise ValueError(f"prefix_len is on {prefix_len.device}, the pools on {device}")
    return prefix_len


def sageattn_splitkv_paged_prefix(q: torch.Tensor, cache, block_table: torch.Tensor, kv_lens: torch.Tensor, prefix,
                                  prefix_table: torch.Tensor, prefix_len: torch.Tensor, num_splits: Optional[int] = None,
                                  prefix_splits: Optional[int] = None, q_fold: int = 1, sm_scale: Optional[float] = None,
                                  return_lse: bool = False):
    """Causal split-KV attention of B sequences that share a prefix, on paged caches over ONE set of pools.  ``cache`` (a
    ``SagePagedKVCache`` or ``SagePagedRowCache`` of B sequences) with ``block_table`` ``[B, max_pages]`` and ``kv_lens``
    ``[B]`` holds the SUFFIXES: they count and address the suffix keys only.  ``prefix`` (a cache of ONE sequence over the same
    pools: ``whole.narrow(0, 1)`` beside ``cache = whole.narrow(1, B)``) with ``prefix_table`` int32 ``[max_prefix_pages]``
    (or its ``[1, max_prefix_pages]`` row) and ``prefix_len`` int32 ``[1]`` holds the shared prefix, with statistics of its
    own.  The valid prefix pages and the valid suffix pages must be distinct (not checked).

    ``q`` is ``[B, Hq, M, D]`` (NHD: ``[B, M, Hq, D]``) as ``sageattn_splitkv_paged(causal=True)`` takes it: ``q_fold`` = g
    divides M, row r is token r // g, and the tokens are the last M / g positions of the suffix.  Row (b, h, m) attends every
    prefix key ``[0, Lp)``, ``Lp = clamp(prefix_len[0], 0, max_prefix_pages * page_size)``, and the suffix keys the causal paged
    operator gives it at ``len_b``.  Three launches: the non-causal paged kernel on the prefix with the B * M query rows folded
    into one batch (``prefix_splits`` splits), the causal paged kernel on the suffixes (``num_splits``), and the merge -- each
    segment's splits as ``sageattn_splitkv_paged`` merges them, then the two segments by their natural-log LSEs, each with its
    own smoothing correction (include/sageattn_hip_prefix.h).

    Where only one segment has keys for a row the row has the bits of the existing operator on that segment: ``Lp = 0`` gives
    ``sageattn_splitkv_paged(causal=True)`` on the suffixes, empty suffixes give the un-folded ``sageattn_splitkv_paged`` on the
    prefix with the folded q.  A row without any key gives o = 0, lse = -inf.  Rows and table entries beyond the lengths
    influence nothing, as in ``sageattn_splitkv_paged``; lengths and tables are read on the device only.

    ``num_splits`` / ``prefix_splits``: 1..16, or None for ``splitkv_num_splits(B, Hq, M, max_pages * page_size)`` /
    ``splitkv_num_splits(1, Hq, B * M, max_prefix_pages * page_size)``.  The folded q is a view for an NHD-contiguous q and for
    M = 1 (and for slices of those along the last dim); any other q travels as one contiguous copy."""
    kinds = tuple(paged._CACHE_TYPES)
    for name, c in (("cache", cache), ("prefix", prefix)):
        if not isinstance(c, kinds):
            raise TypeError(f"{name} must be a SagePagedKVCache or a SagePagedRowCache, got {type(c).__name__}")
    _check_shared_pools(cache, prefix)
    if prefix.km.size(0) != 1:
        raise ValueError(f"prefix must be a cache of one sequence (whole.narrow(0, 1)), got {prefix.km.size(0)} sequences")
    block_table = paged._check_block_table(block_table, q.size(0), cache.device)
    prefix_table = _check_prefix_table(prefix_table, cache.device)
    prefix_len = _check_prefix_len(prefix_len, cache.device)
    if kv_lens is None:
        raise TypeError("kv_lens must be an int32 tensor of shape [B]")
    kv_lens, ns, M = core._splitkv_front("sageattn_splitkv_paged_prefix", True, q, cache.k8, cache.k8, kv_lens, num_splits,
                                         cache.tensor_layout, cache.pv, cache.qk_quant_gran, {})
    if prefix_splits is not None:
        if isinstance(prefix_splits, bool) or not isinstance(prefix_splits, int):
            raise TypeError(f"prefix_splits must be an int in [1, {core.SPLITKV_MAX}] or None, got {type(prefix_splits).__name__}")
        if not 1 <= prefix_splits <= core.SPLITKV_MAX:
            raise ValueError(f"prefix_splits must be in [1, {core.SPLITKV_MAX}] (or None: from the shape), got {prefix_splits}")
    if isinstance(q_fold, bool) or not isinstance(q_fold, int):
        raise TypeError(f"q_fold must be an int >= 1, got {type(q_fold).__name__}")
    if q_fold < 1 or M % q_fold != 0:
        raise ValueError(f"q_fold must be >= 1 and divide the {M} query rows, got {q_fold}")
    if q.dtype != cache.dtype or q.device != cache.device:
        raise ValueError("q must have the dtype and device of the cache")
    D = cache.head_dim
    if q.size(-1) != D:
        raise ValueError(f"q must have the cache's head_dim {D}, got {q.size(-1)}")
    B, Hq = L.dims(q, cache.tensor_layout)[:2]
    Hk = cache.num_kv_heads
    if Hq % Hk != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by num_kv_heads ({Hk})")
    if cache.km.size(0) != B:
        raise ValueError(f"q has {B} sequences, the cache {cache.km.size(0)}")
    if num_splits is None:  # (from the logical capacity: the pool's third dim is one page)
        ns = core.splitkv_num_splits(B, Hq, M, block_table.size(1) * cache.page_size)
    if prefix_splits is None:
        prefix_splits = core.splitkv_num_splits(1, Hq, B * M, prefix_table.size(0) * cache.page_size)
    if sm_scale is None:
        sm_scale = D ** -0.5
    fp8 = cache.pv == "fp8"
    op = getattr(torch.ops.sageattention_amd_prefix, f"attn_splitkv_paged_prefix{'_lse' if return_lse else ''}")
    return op(q, cache.k8, cache.k_scale, cache.km, cache.v8 if fp8 else _v_pool(cache), cache.v_scale if fp8 else None,
              block_table, kv_lens, prefix_table, prefix_len, prefix.km, prefix.v_scale if fp8 else None, ns, prefix_splits,
              q_fold, cache.tensor_layout, float(sm_scale), cache.qk_quant_gran)
