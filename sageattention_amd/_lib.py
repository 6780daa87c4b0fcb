"""ctypes binding of the C-ABI library ``libsageattn_hip.so`` (include/sageattn_hip.h).

PyTorch is plumbing only: it owns device memory and the current HIP stream; every compute step of the
hot path goes through the C ABI.  There is NO CPU or eager fallback: if the library is missing or the
call fails, this raises."""
import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_size_t, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsageattn_hip.so")

SAGE_F16, SAGE_BF16 = 0, 1
GRAN_PER_BLOCK, GRAN_PER_WARP, GRAN_PER_THREAD = 1, 2, 3
ROUND_TRITON, ROUND_CUDA = 0, 1
SELECT_CDF, SELECT_TOPK = 0, 1  # SAGE_SELECT_*: the rule of sage_block_select


class SageTensor(ctypes.Structure):
    _fields_ = [("data", c_void_p), ("stride_b", c_int64), ("stride_h", c_int64), ("stride_n", c_int64)]


class KvLayout(ctypes.Structure):
    """sage_kv_layout (include/sageattn_hip.h): tile strides of k8 / v and the strides of the k scales."""
    _fields_ = [("k_tile_stride", c_int64), ("v_tile_stride", c_int64), ("ks_stride_b", c_int64),
                ("ks_stride_h", c_int64), ("ks_stride_tile", c_int64)]


class OpOpts(ctypes.Structure):
    """sage_op_opts (include/sageattn_hip.h)"""
    _fields_ = [("qk_gran", c_int), ("warpq", c_int), ("smooth_k", c_int), ("fuse_q", c_int), ("nwaves", c_int),
                ("reserved", c_int * 3)]


_P = ctypes.POINTER(SageTensor)
_PO = ctypes.POINTER(OpOpts)
_PL = ctypes.POINTER(KvLayout)
_P64 = ctypes.POINTER(c_int64)  # a host array of strides
_I, _V = c_int, c_void_p        # _V: a device pointer, or the stream
_lib = None

# name -> (restype, argtypes); must list every symbol include/sageattn_hip.h declares, with its types
# (tests/test_bindings.py compares both with the header's prototypes)
SIGNATURES = {
    "sage_abi_version": (_I, []),
    "sage_status_string": (c_char_p, [_I]),
    "sage_target_arch": (c_char_p, []),
    "sage_set_tuning": (_I, [_I, _I]),
    "sage_get_tuning": (_I, [_I]),
    "sage_k_mean": (_I, [_P, _I, _I, _I, _I, _I, _V, _V, _V]),
    "sage_quant_qk_int8": (_I, [_P, _I, _I, _I, _I, _I, _V, _P, _V, _I, _I, _I, _I, c_float, _I, _V, _I, _V, _V]),
    "sage_sub_mean_f16": (_I, [_P, _I, _I, _I, _I, _I, _V, _P, _V]),
    "sage_quant_v_fp8": (_I, [_P, _I, _I, _I, _I, _I, _P, _V, _V, c_float, _V, _V]),
    "sage_quant_qk_int8_varlen": (_I, [_P, _I, _V, _I, _I, _I, _I, _V, _P, _V, _I, _I, _I, _I, c_float, _I, _V]),
    "sage_merge_attn_states": (_I, [_V, _V, _V, _I, _V, c_int64, _I, _V]),
    "sage_merge_attn_states_multi": (_I, [_V, _V, _I, _I, _V, _V, c_int64, _I, _V]),
    "sage_merge_attn_states_multi_ex": (_I, [_V, _V, _I, _I, _V, _V, c_int64, _I, c_float, _V, c_float, _V]),
    "sage_finish_lse": (_I, [_V, _V, c_float, _V, c_int64, _V]),
    "sage_sageattn_workspace_bytes": (c_size_t, [_I, _I, _I, _I, _I, _I, _I, _I, _PO]),
    "sage_sageattn_pv_f16": (_I, [_P, _P, _P, _I, _P, _V, _I, _I, _I, _I, _I, _I, _I, c_float, _PO, _V, c_size_t, _V]),
    "sage_sageattn_pv_f8": (_I, [_P, _P, _P, _I, _P, _V, _I, _I, _I, _I, _I, _I, _I, c_float, c_float, _PO, _V, c_size_t,
                                 _V]),
    "sage_k_smooth_quant": (_I, [_P, _I, _I, _I, _I, _I, _P, _V, _V, _I, _I, _V, _V]),
    "sage_kv_prepare_fp8": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _V, _V, _I, _I, _P, _V, c_float, _V, _V]),
    "sage_seq_stats": (_I, [_P, _I, _I, _I, _I, _I, _V, _V, _V]),
    "sage_kv_stats_reduce": (_I, [_V, _V, _I, c_int64, _I, _I, c_int64, _I, c_float, _V, _V, _V, _V]),
    "sage_quant_k_int8_kvtiles": (_I, [_P, _I, _I, _I, _I, _I, _V, _P, c_int64, _V, _P64, _I, _I, _V]),
    "sage_quant_v_fp8_apply": (_I, [_P, _I, _I, _I, _I, _I, _P, c_int64, _V, _V]),
    "sage_block_map_compact": (_I, [_V, _P64, _I, _I, _I, _I, _V, c_int64, _V]),
    "sage_splitkv_workspace_bytes": (c_size_t, [_I, _I, _I, _I, _I]),
    "sage_block_pool_sim": (_I, [_P, _I, _I, _I, _I, _I, _I, _V, _V, _V, _V]),
    "sage_block_select_cdf": (_I, [_V, _V, _V, _V, _I, _I, _I, _I, _I, _I, c_float, _V, _V, _V, c_int64, _V, _V]),
    # ... with (rule, rule_param, keep_first, keep_last) in the place of cdfthreshd
    "sage_block_select": (_I, [_V, _V, _V, _V, _I, _I, _I, _I, _I, _I, c_float, _V, _I, _V, _I, _I, _V, c_int64, _V, _V]),
    # the Q / K arguments of sage_attn_qk_int8_pv_f16, then mass
    "sage_attn_tile_mass": (_I, [_P, _P, _V, _V, _I, _I, _I, _I, _I, _I, _I, _I, _I, c_float, _I, _V, _V]),
    "sage_block_plan_recall": (_I, [_V, c_int64, _V, _I, _I, _I, _I, _V, _V, _V]),
}
for _name in ("sage_k_mean", "sage_quant_v_fp8", "sage_kv_prepare_fp8", "sage_seq_stats", "sage_block_sparse"):
    SIGNATURES[_name + "_workspace_bytes"] = (c_size_t, [_I, _I, _I, _I])
# per-batch key lengths on the pre-pass, predictor and calibration entries: the twin's arguments, then kv_lens in front of
# the stream
for _name in ("sage_k_smooth_quant", "sage_kv_prepare_fp8", "sage_block_pool_sim", "sage_block_select", "sage_attn_tile_mass",
              "sage_block_plan_recall"):
    SIGNATURES[_name + "_kvlen"] = (_I, SIGNATURES[_name][1][:-1] + [_V, _V])

# The attention entry points.  Four families: the operands up to lse, then B, Hq, Hk, M, N, D, [is_causal,] the quantization
# arguments, whatever the form appends, and the stream.
_OPERANDS = {
    "qk_int8_pv_f16": [_P, _P, _P, _I, _P, _I] + [_V] * 4,       # q8 k8 v v_dtype o o_dtype | q_scale k_scale v_mean lse
    "qk_int8_pv_f8": [_P, _P, _P, _P, _I] + [_V] * 5,            # q8 k8 v_fp8 o o_dtype | q_scale k_scale v_scale v_mean lse
    "fusedq_pv_f16": [_P, _I, _P, _P, _I, _P, _I] + [_V] * 4,    # q q_dtype k8 v v_dtype o o_dtype | k_scale km v_mean lse
    "fusedq_pv_f8": [_P, _I, _P, _P, _P, _I] + [_V] * 5,         # q q_dtype k8 v_fp8 o o_dtype | k_scale km v_scale v_mean lse
}
_QUANT = {"qk_int8": [_I, _I, _I, c_float, _I],   # qk_gran blkq warpq sm_scale logit_mult_is_one
          "fusedq": [_I, _I, c_float]}            # qk_gran warpq sm_scale


def _attn(family, appended=(), operands=None, is_causal=True, quant=None):
    operands = _OPERANDS[family] if operands is None else operands
    quant = _QUANT[family.split("_pv_")[0]] if quant is None else quant
    return (_I, operands + [_I] * 6 + [_I] * is_causal + quant + list(appended) + [_V])


_LISTS = [_V, c_int64]                     # block_lists, block_lists_bytes
_PVSKIP = _LISTS + [_V, _V]                # ... pv_thresh, skipped
_SPLITKV = [_V, _I, _V, c_size_t]          # kv_lens (or NULL), num_splits, workspace, workspace_bytes
_FORMS = {"": [], "_blocksparse": _LISTS, "_blocksparse_pvskip": _PVSKIP, "_kvlen": [_V], "_blocksparse_kvlen": _PVSKIP + [_V]}
for _family in _OPERANDS:
    for _form, _appended in _FORMS.items():
        SIGNATURES[f"sage_attn_{_family}{_form}"] = _attn(_family, _appended)
    if _family.startswith("fusedq"):   # split-KV: no is_causal; the causal form has q_fold behind num_splits
        SIGNATURES[f"sage_attn_{_family}_splitkv"] = _attn(_family, _SPLITKV, is_causal=False)
        SIGNATURES[f"sage_attn_{_family}_splitkv_causal"] = _attn(_family, _SPLITKV[:2] + [_I] + _SPLITKV[2:], is_causal=False)
    else:                              # an explicit tile layout: kv_layout in the place of v_mean, no logit_mult_is_one
        SIGNATURES[f"sage_attn_{_family}_kvtiles"] = _attn(_family, operands=_OPERANDS[_family][:-2] + [_PL, _V],
                                                           quant=_QUANT["qk_int8"][:-1])
# packed sequences: cu_seqlens_q, cu_seqlens_k in the place of v_mean, lse; num_seqs and the two max_seqlen among the sizes
SIGNATURES["sage_attn_qk_int8_pv_f16_varlen"] = _attn("qk_int8_pv_f16")
# attn_mask, mask_kind, mask_strides in the place of v_mean; no is_causal
SIGNATURES["sage_attn_qk_int8_pv_f16_masked"] = _attn(
    "qk_int8_pv_f16", operands=_OPERANDS["qk_int8_pv_f16"][:-2] + [_V, _I, _P64, _V], is_causal=False)


# The extension headers, one table each: SIGNATURES stays the list of include/sageattn_hip.h.
# include/sageattn_hip_kvcache.h: k v dtype | B H N D | km k_int8 k_scale gran rounding | v_fp8 v_coef | start_lens kv_lens
# max_new stream
KVCACHE_SIGNATURES = {
    "sage_kv_cache_append": (_I, [_P, _P, _I, _I, _I, _I, _I, _V, _P, _V, _I, _I, _P, _V, _V, _V, _I, _V]),
}

# include/sageattn_hip_paged.h.  The table's own arguments, in this order in all three: block_table table_stride max_pages
# page_size num_pages.  The append: k_pool v_pool dtype | B H D | km k8_pool k_scale_pool gran rounding | v8_pool v_coef | table |
# start_lens kv_lens max_new stream.  The attention entries: the fusedq operands without v_mean | B Hq Hk M D | qk_gran warpq
# sm_scale | table | kv_lens num_splits causal q_fold workspace workspace_bytes stream
_TABLE = [_V, c_int64, _I, _I, _I]
_PAGED_TAIL = [_I] * 5 + _QUANT["fusedq"] + _TABLE + [_V, _I, _I, _I, _V, c_size_t, _V]
PAGED_SIGNATURES = {
    "sage_kv_cache_append_paged": (_I, [_P, _P, _I, _I, _I, _I, _V, _P, _V, _I, _I, _P, _V] + _TABLE + [_V, _V, _I, _V]),
    "sage_attn_fusedq_pv_f16_splitkv_paged": (_I, [_P, _I, _P, _P, _I, _P, _I, _V, _V, _V] + _PAGED_TAIL),
    "sage_attn_fusedq_pv_f8_splitkv_paged": (_I, [_P, _I, _P, _P, _P, _I, _V, _V, _V, _V] + _PAGED_TAIL),
}

# include/sageattn_hip_paged_rows.h: k_new v_new dtype | B H T D | km k_tail k8_pool k_scale_pool gran rounding | v_pool v8_pool
# v_coef | table | start_lens kv_lens stream
PAGED_ROWS_SIGNATURES = {
    "sage_kv_cache_append_rows_paged": (_I, [_P, _P, _I, _I, _I, _I, _I, _V, _V, _P, _V, _I, _I, _P, _P, _V] + _TABLE + [_V, _V, _V]),
}

# include/sageattn_hip_prefix.h.  The attention entries: the operands of the paged ones | B Hq Hk M D | qk_gran warpq sm_scale |
# table | kv_lens | prefix_table max_prefix_pages prefix_len km_p [v_scale_p] | prefix_splits num_splits q_fold workspace
# workspace_bytes stream
_PREFIX_HEAD = [_I] * 5 + _QUANT["fusedq"] + _TABLE + [_V] + [_V, _I, _V, _V]
_PREFIX_TAIL = [_I, _I, _I, _V, c_size_t, _V]
PREFIX_SIGNATURES = {
    "sage_prefix_workspace_bytes": (c_size_t, [_I] * 6),
    "sage_attn_fusedq_pv_f16_splitkv_paged_prefix": (_I, [_P, _I, _P, _P, _I, _P, _I, _V, _V, _V] + _PREFIX_HEAD + _PREFIX_TAIL),
    "sage_attn_fusedq_pv_f8_splitkv_paged_prefix": (_I, [_P, _I, _P, _P, _P, _I, _V, _V, _V, _V] + _PREFIX_HEAD + [_V] + _PREFIX_TAIL),
}


def bind(cdll, missing_ok=True):
    """Set restype / argtypes on every SIGNATURES, KVCACHE_SIGNATURES, PAGED_SIGNATURES, PAGED_ROWS_SIGNATURES and
    PREFIX_SIGNATURES symbol ``cdll`` has and return it.  An older library
    loaded for an A/B run may lack some; with ``missing_ok=False`` (the package's own library) a missing symbol raises
    AttributeError."""
    for name, (res, args) in {**SIGNATURES, **KVCACHE_SIGNATURES, **PAGED_SIGNATURES, **PAGED_ROWS_SIGNATURES,
                              **PREFIX_SIGNATURES}.items():
        fn = getattr(cdll, name, None) if missing_ok else getattr(cdll, name)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return cdll


def lib():
    """Load the HIP library (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the gfx950 HIP library has not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `python sageattention_amd/_build.py`). "
                "There is no CPU fallback for the SageAttention hot path.")
        _lib = l = bind(ctypes.CDLL(LIB_PATH), missing_ok=False)
        if os.environ.get("SAGE_NWAVES"):  # tuning knob (speed only): waves per attention workgroup, 4 or 8
            l.sage_set_tuning(0, int(os.environ["SAGE_NWAVES"]))
    return _lib


def check(status: int, what: str):
    """Map sage_status to the reference's exception types (TORCH_CHECK -> RuntimeError,
    std::invalid_argument -> ValueError)."""
    if status == 0:
        return
    msg = f"{what}: {lib().sage_status_string(status).decode()} (status {status})"
    if status in (-1, -2):
        raise ValueError(msg)
    raise RuntimeError(msg)


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float16:
        return SAGE_F16
    if dt == torch.bfloat16:
        return SAGE_BF16
    raise ValueError(f"unsupported dtype {dt}")


def desc(t: torch.Tensor, tensor_layout: str) -> SageTensor:
    """[B,H,N,D] descriptor of a 4-D tensor in either reference layout (core.py:585)."""
    assert t.dim() == 4 and t.stride(-1) == 1, "Last dim must be contiguous."
    if tensor_layout == "HND":
        return SageTensor(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))
    if tensor_layout == "NHD":
        return SageTensor(t.data_ptr(), t.stride(0), t.stride(2), t.stride(1))
    raise ValueError(f"Unknown tensor layout: {tensor_layout}")


def desc_vt(v8: torch.Tensor, tensor_layout: str) -> SageTensor:
    """Descriptor of the FP8 V^T of ``per_channel_fp8`` / ``kv_prepare_fp8``, [B,Hk,D,Npad] (HND) or [B,D,Hk,Npad] (NHD):
    stride_n is the stride of the d index."""
    if tensor_layout == "HND":
        return SageTensor(v8.data_ptr(), v8.stride(0), v8.stride(1), v8.stride(2))
    return SageTensor(v8.data_ptr(), v8.stride(0), v8.stride(2), v8.stride(1))


def dims(t: torch.Tensor, tensor_layout: str):
    """-> (B, H, N, D)"""
    if tensor_layout == "HND":
        return t.size(0), t.size(1), t.size(2), t.size(3)
    if tensor_layout == "NHD":
        return t.size(0), t.size(2), t.size(1), t.size(3)
    raise ValueError(f"Unknown tensor layout: {tensor_layout}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(device) -> int:
    """hipStream_t of torch's current stream on `device` (the raw getter is ~10x cheaper than building a Stream object:
    4 us of the ~40 us a call costs on the host)."""
    if _raw_stream is not None and device.index is not None:
        return _raw_stream(device.index)
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()
